#!/usr/bin/env python3
"""Counts the epilogue's instructions in a device assembly listing (`make -C ws_unet_amd/csrc isa`).

    python tools/epilogue_isa.py ws_unet_amd/csrc/isa/conv3x3_q.s [--hist SUBSTRING]

A kernel's epilogue is taken to be every basic block that holds a `buffer_store_dwordx4` or a `global_store_dword` (the planar stores and the
head's planes) and the block each of them falls through to (the range flag's maximum is computed behind the test of its pointer): per kernel the table gives those blocks' VALU / MFMA / store counts, their number, and a few opcode counts; --hist prints
the whole opcode histogram of the kernels whose demangled name contains SUBSTRING.  (The loader waves store nothing, so their blocks never count.)
"""
import argparse
import collections
import re
import subprocess
import sys

WATCH = ("v_max_f32", "v_max3_f32", "v_pk_max_u16", "v_and_b32", "v_cndmask_b32", "v_add_u32", "v_lshl_add_u32", "v_mov_b32", "v_permlane32_swap")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path, waitcnt_operands=False):
    """{symbol: [[opcode, ...] per basic block]} for every .amdhsa kernel body of the listing.  waitcnt_operands: an `s_waitcnt` keeps its
    operands (`s_waitcnt lgkmcnt(4)`, one space between the words), every other instruction is its opcode alone"""
    res, cur, name = {}, None, None
    lab = re.compile(r"^([A-Za-z_.$][\w.$]*):")
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if not line:
            continue
        m = lab.match(line)
        if m:
            if not m.group(1).startswith(".L"):
                name = m.group(1)
                cur = res.setdefault(name, [[]])
            elif cur is not None:
                cur.append([])
            continue
        s = line.strip()
        if s.startswith(".") or cur is None:
            if s.startswith(".end_amdhsa_kernel") or s.startswith(".section"):
                cur = None
            continue
        op = s.split()[0]
        cur[-1].append(" ".join(s.split()) if waitcnt_operands and op == "s_waitcnt" else op)
        if op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm"):
            cur.append([])
    return res


def is_store(op):
    return op.startswith("buffer_store") or op.startswith("global_store")


def epilogue_blocks(blocks):
    st = [any(op.startswith("buffer_store_dwordx4") or op.startswith("global_store_dword") for op in b) for b in blocks]
    # ... and the block a storing block falls through to: the range flag's reduction sits behind the `a.range_flag != nullptr` branch
    return [b for i, b in enumerate(blocks) if st[i] or (i > 0 and st[i - 1] and b and not b[0].startswith("s_endpgm"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("--hist", default=None)
    args = ap.parse_args()
    ks = {k: v for k, v in kernels(args.listing).items() if any(epilogue_blocks(v))}
    names = demangle(list(ks))
    print("| kernel | blocks | VALU | MFMA | stores | " + " | ".join(WATCH) + " |")
    print("|---|---|---|---|---|" + "---|" * len(WATCH))
    for k, blocks in ks.items():
        eb = epilogue_blocks(blocks)
        ops = collections.Counter(op for b in eb for op in b)
        valu = sum(n for op, n in ops.items() if op.startswith("v_") and not op.startswith("v_mfma"))
        mfma = sum(n for op, n in ops.items() if op.startswith("v_mfma"))
        st = sum(n for op, n in ops.items() if is_store(op))
        short = names[k].replace("void ", "").replace("(QArgs)", "").replace("(anonymous namespace)::", "")
        print(f"| `{short}` | {len(eb)} | {valu} | {mfma} | {st} | " + " | ".join(str(sum(n for op, n in ops.items() if op.startswith(w))) for w in WATCH) + " |")
        if args.hist is not None and args.hist in names[k]:
            for op, n in sorted(ops.items(), key=lambda t: -t[1]):
                print(f"    {n:5d} {op}", file=sys.stderr)


if __name__ == "__main__":
    main()
