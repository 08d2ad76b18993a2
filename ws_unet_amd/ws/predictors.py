"""The model names of the WS drivers (ws.estimate, ws.roc, ws.locate, ws.keysearch), in one table: which names a kind of predictor
answers and how it makes a fresh estimator for one.  A name that no entry answers is a trained UNet run's (ws.estimate.resolve_predictor).
A new predictor is its own module and one line of TABLE; what the statistic kernels get from it is its `device_arguments` method
(ws.estimate.predictor_arguments)."""
from __future__ import annotations

import collections

from .. import filters, ols, ols5
from . import jpeg, structural

# names: () -> the names answered now, in the order they are listed (the registries grow at run time: --kernels, --kernels5);
# make: name -> a fresh estimator; pixel: False for the structural estimators, which are no pixel predictors
Entry = collections.namedtuple("Entry", "names make pixel", defaults=(True,))
TABLE = [
    Entry(lambda: sorted(structural.NAMES), structural.StructuralEstimator, pixel=False),      # 'SPA' / 'RS'
    Entry(lambda: sorted(ols.ADAPTIVE_NAMES), ols.adaptive_estimator),                         # the 3x3 least-squares fit of each image
    Entry(ols5.names, ols5.estimator),                                                         # the 5x5 one, then the --kernels5 names
    Entry(lambda: sorted(jpeg.NAMES), jpeg.estimator),                                         # the recompression predictor
    Entry(lambda: sorted(filters.NAMED_FILTERS_2D), lambda name: filters.get_filter_estimator(filter_name=name, flatten=False)),
]


def by_name(name):
    """A fresh estimator for a model name, from the first entry of TABLE that answers it; None for a name nobody answers."""
    for entry in TABLE:
        if name in entry.names():
            return entry.make(name)
    return None


def names(pixel_only: bool = False) -> list:
    """Every answered name, grouped in TABLE's order; with pixel_only without the structural estimators."""
    return [name for entry in TABLE if entry.pixel or not pixel_only for name in entry.names()]


def require(name):
    """`by_name`, or the caller's error for a name nobody answers."""
    estimator = by_name(name)
    if estimator is None:
        raise ValueError(f"unknown filter {name!r}; choose from {names()}")
    return estimator


def filters_help(structural: bool) -> str:
    """The help sentence of a driver's --filters; structural: the driver also takes the structural estimators."""
    text = "pixel predictors by name: " + ", ".join(repr(n) for n in names(pixel_only=True)) + ", and the names of a --kernels / --kernels5 file"
    if structural:
        text += "; the structural estimators " + " / ".join(repr(n) for n in names() if n not in names(pixel_only=True))
    return text


def add_arguments(ap) -> None:
    """The drivers' --kernels and --kernels5."""
    ols.add_kernels_argument(ap)
    ols5.add_kernels_argument(ap)


def register_from_args(a) -> None:
    ols.register_from_args(a)
    ols5.register_from_args(a)
