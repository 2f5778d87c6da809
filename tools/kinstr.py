"""Static instruction counts of one kernel in a `hipcc -S` assembly file.

Usage: python tools/kinstr.py <file.s> <kernel-name substring> [...]

For every kernel whose symbol contains the substring: the instruction
count, its split by class (from the mnemonic's prefix alone) and the
same split for the part before the first s_barrier.
"""
import re
import sys

CLASSES = ["v_mfma", "v_cndmask", "v_cmp", "lane moves", "other v_", "ds_",
           "global_/buffer_", "s_waitcnt", "branches", "other scalar",
           "other"]


def classify(m):
    if m.startswith("v_mfma"):
        return "v_mfma"
    if m.startswith("v_cndmask"):
        return "v_cndmask"
    if m.startswith("v_cmp"):
        return "v_cmp"
    if m.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane moves"
    if m.startswith("v_"):
        return "other v_"
    if m.startswith("ds_"):
        return "ds_"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "global_/buffer_"
    if m.startswith("s_waitcnt"):
        return "s_waitcnt"
    if m.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc",
                     "s_endpgm")):
        return "branches"
    if m.startswith("s_"):
        return "other scalar"
    return "other"


def kernels(path):
    """(symbol, [mnemonic, ...]) of every function body in the file."""
    name, body = None, []
    label = re.compile(r"^([A-Za-z_.$][\w.$]*):")
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if not line:
            continue
        m = label.match(line)
        if m:
            if not m.group(1).startswith(".") and name is None:
                name, body = m.group(1), []
            continue
        s = line.strip()
        if s.startswith(".") or name is None:
            if s.startswith(".Lfunc_end") or s.startswith(".size"):
                if name is not None and body:
                    yield name, body
                name, body = None, []
            continue
        body.append(s.split()[0])
    if name is not None and body:
        yield name, body


def table(mn):
    t = dict.fromkeys(CLASSES, 0)
    for m in mn:
        t[classify(m)] += 1
    return t


def main():
    path, subs = sys.argv[1], sys.argv[2:]
    for name, mn in kernels(path):
        if not any(s in name for s in subs):
            continue
        bar = next((i for i, m in enumerate(mn) if m.startswith("s_barrier")),
                   len(mn))
        whole, pre = table(mn), table(mn[:bar])
        print(name)
        print("  %-18s %6s %14s" % ("class", "total", "before barrier"))
        print("  %-18s %6d %14d" % ("instructions", len(mn), bar))
        for c in CLASSES:
            if whole[c]:
                print("  %-18s %6d %14d" % (c, whole[c], pre[c]))


if __name__ == "__main__":
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    main()
