"""WS payload estimator built on the pixel predictor (reference src/ws/__init__.py:7), and `ws.roc`, its detection ROC / AUC tables
(the B0 detector of the reference's roc.py is out of scope: its scores enter as files)."""
from . import estimate  # noqa: F401
