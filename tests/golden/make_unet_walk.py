#!/usr/bin/env python3
"""Write tests/golden/unet_walk.json: per configuration of tests/walk_recorder.py the C-ABI call trace of two consecutive steps and the
SHA-256 digest of the output.  Run on the GPU, on the commit whose host layer is the yardstick:

    python tests/golden/make_unet_walk.py [out.json]

Every configuration is recorded twice, each time with a freshly built model.  The two traces must be equal; a digest is kept only where the
two runs agree (null otherwise).
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import walk_recorder as wr  # noqa: E402


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "unet_walk.json"
    res, unstable = {}, []
    for name, cfg in wr.configs().items():
        a, b = wr.record(cfg), wr.record(cfg)
        assert a["trace"] == b["trace"], f"{name}: two runs of the same tree made different calls"
        if a["digest"] != b["digest"]:
            unstable.append(name)
            a["digest"] = None
        res[name] = a
    out.write_text(json.dumps(res, indent=0) + "\n")
    calls = sum(len(v["trace"]) for v in res.values())
    print(f"{out}: {len(res)} configurations, {calls} calls, {out.stat().st_size // 1024} KiB; digests that differ between two runs: {unstable or 'none'}")


if __name__ == "__main__":
    main()
