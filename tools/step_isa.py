#!/usr/bin/env python3
"""Counts the instructions of the chunk steps in a device assembly listing (`make -C ws_unet_amd/csrc isa`).

    python tools/step_isa.py ws_unet_amd/csrc/isa/conv3x3_q.s [--min-mfma N] [--kernel SUBSTRING] [--list OPCODE_PREFIX] [--stream]

A chunk step of the planar convs is one basic block: its matrix instructions and everything the step issues beside them.  For every kernel of
the listing the table gives each basic block with at least N (default 8) matrix instructions: MFMA, VALU (vector ALU without the matrix
instructions), `v_cndmask`, the address adds (`v_add_u32`, `v_lshl_add_u32`, `v_add3_u32`), `ds_*`, stores and barriers.  A block with stores is
a tile's last step together with its epilogue; one without is a steady step.  --list prints the instructions of the counted blocks whose opcode
starts with the prefix (what is left of a kind, and where).  --stream prints, per counted block, the order of its fragment reads, waits and
matrix instructions behind the barrier: r = `ds_read_b128`, s = a smaller LDS read, M = matrix instruction, [n] = `s_waitcnt lgkmcnt(n)`
(`[]` for n = 0) -- whether a unit's reads stand in front of the previous unit's matrix instructions (the wait then leaves n reads in
flight) or in front of their own (`[]`: the wave waits out its own LDS latency).  The block parser is tools/epilogue_isa.py's."""
import argparse
import collections
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import epilogue_isa  # noqa: E402

ADDS = ("v_add_u32", "v_lshl_add_u32", "v_add3_u32")
COLUMNS = ("MFMA", "VALU", "v_cndmask", "adds", "ds", "stores", "barriers")


LGKM = re.compile(r"lgkmcnt\((\d+)\)")


def is_mfma(op):
    return op.startswith("v_mfma")


def is_valu(op):
    return op.startswith("v_") and not is_mfma(op)


def count(block):
    """the table's columns for one basic block (a list of opcodes)"""
    ops = collections.Counter(block)
    pick = lambda pred: sum(n for op, n in ops.items() if pred(op))
    return {
        "MFMA": pick(is_mfma),
        "VALU": pick(is_valu),
        "v_cndmask": pick(lambda op: op.startswith("v_cndmask")),
        "adds": pick(lambda op: op.startswith(ADDS)),
        "ds": pick(lambda op: op.startswith("ds_")),
        "stores": pick(epilogue_isa.is_store),
        "barriers": pick(lambda op: op == "s_barrier"),
    }


def step_blocks(blocks, min_mfma=8):
    """[(block index, counts, opcodes)] of the blocks with at least min_mfma matrix instructions"""
    out = []
    for i, b in enumerate(blocks):
        c = count(b)
        if c["MFMA"] >= min_mfma:
            out.append((i, c, b))
    return out


def lgkm_wait(op):
    """the lgkmcnt operand of an `s_waitcnt` kept with its operands (steps(..., waitcnt_operands=True)); None: another instruction, or a wait on
    other counters only"""
    if not op.startswith("s_waitcnt"):
        return None
    m = LGKM.search(op)
    return int(m.group(1)) if m else None


def step_waits(block):
    """[(lgkmcnt operand, a matrix instruction follows before the next wait)] for the LDS waits between a block's barrier and its last matrix
    instruction -- a step's fragment waits"""
    start = block.index("s_barrier") + 1 if "s_barrier" in block else 0
    last = max(i for i, op in enumerate(block) if is_mfma(op))
    out = []
    for i in range(start, last):
        n = lgkm_wait(block[i])
        if n is None:
            continue
        nxt = next((op for op in block[i + 1:last + 1] if is_mfma(op) or lgkm_wait(op) is not None), None)
        out.append((n, nxt is not None and is_mfma(nxt)))
    return out


def stream(block):
    """the block behind its barrier as a string of r / s / M / [n] (see the module's text), up to its last matrix instruction"""
    start = block.index("s_barrier") + 1 if "s_barrier" in block else 0
    last = max(i for i, op in enumerate(block) if is_mfma(op))
    out = []
    for op in block[start:last + 1]:
        n = lgkm_wait(op)
        if is_mfma(op):
            out.append("M")
        elif op.startswith("ds_read_b128"):
            out.append("r")
        elif op.startswith("ds_read"):
            out.append("s")
        elif n is not None:
            out.append("[%s]" % (n or ""))
    return "".join(out)


def short_name(demangled):
    return demangled.replace("void ", "").replace("(anonymous namespace)::", "").replace("(QArgs)", "").replace("(UArgs)", "")


def steps(path, min_mfma=8, waitcnt_operands=False):
    """{demangled kernel name: [(block index, counts, opcodes)]} for the kernels that have a step block; waitcnt_operands: the opcode lists keep
    every `s_waitcnt` with its operands (step_waits, stream)"""
    ks = {k: step_blocks(v, min_mfma) for k, v in epilogue_isa.kernels(path, waitcnt_operands).items()}
    ks = {k: v for k, v in ks.items() if v}
    names = epilogue_isa.demangle(list(ks))
    return {short_name(names[k]): v for k, v in ks.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--min-mfma", type=int, default=8)
    ap.add_argument("--kernel", default=None, help="only kernels whose demangled name contains this")
    ap.add_argument("--list", default=None, metavar="PREFIX", help="print the counted blocks' opcodes that start with PREFIX")
    ap.add_argument("--stream", action="store_true", help="print the counted blocks' reads, waits and matrix instructions in order")
    args = ap.parse_args()
    print("| kernel | block | " + " | ".join(COLUMNS) + " |")
    print("|---|---|" + "---|" * len(COLUMNS))
    for name, rows in steps(args.listing, args.min_mfma, waitcnt_operands=True).items():
        if args.kernel is not None and args.kernel not in name:
            continue
        for i, c, b in rows:
            print(f"| `{name}` | {i} | " + " | ".join(str(c[col]) for col in COLUMNS) + " |")
            if args.stream:
                print(f"    {stream(b)}", file=sys.stderr)
            if args.list is not None:
                hist = collections.Counter(op for op in b if op.startswith(args.list))
                for op, n in sorted(hist.items(), key=lambda t: -t[1]):
                    print(f"    {n:5d} {op}", file=sys.stderr)


if __name__ == "__main__":
    main()
