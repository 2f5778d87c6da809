"""Static instruction counts of one kernel in a `hipcc -S` assembly file.

Usage: python tools/kinstr.py <file.s> <kernel-name substring> [...]

For every kernel whose symbol contains the substring: the instruction
count, its split by class (from the mnemonic's prefix alone) and the
same split for the part before the first s_barrier.

       python tools/kinstr.py --blocks <file.s> <kernel-name substring>

The kernel's basic blocks instead: first instruction, label, count and
the branch (with its target) or barrier that ends each. A kernel that
dispatches on the block index has one barrier per role; the executed
length of a role is the sum of the blocks on its path.
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


def kernels(path, labels=False):
    """(symbol, [mnemonic, ...]) of every function body in the file.
    labels: local labels (.LBB...) stay in the list as "label:" and a
    branch keeps its target ("s_cbranch_scc1 .LBB7_12")."""
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
            elif labels and name is not None:
                body.append(m.group(1) + ":")
            continue
        s = line.strip()
        if s.startswith(".") or name is None:
            if s.startswith(".Lfunc_end") or s.startswith(".size"):
                if name is not None and body:
                    yield name, body
                name, body = None, []
            continue
        f = s.split()
        body.append(" ".join(f[:2]) if labels and is_branch(f[0]) else f[0])
    if name is not None and body:
        yield name, body


def is_branch(m):
    return m.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc",
                         "s_endpgm"))


def blocks(mn):
    """Basic blocks of a labelled body (kernels(..., labels=True)):
    (index of the first instruction, label or "", instruction count,
    terminating branch with its target, or "" when it falls through).
    A barrier ends a block as well, so the counts on either side of it
    can be added up along a path read off the branch targets."""
    out, n, first, lab, cnt = [], 0, 0, "", 0
    for m in mn:
        if m.endswith(":"):
            if cnt:
                out.append((first, lab, cnt, ""))
            first, lab, cnt = n, m[:-1], 0
            continue
        n += 1
        cnt += 1
        if is_branch(m.split()[0]) or m.startswith("s_barrier"):
            out.append((first, lab, cnt, m))
            first, lab, cnt = n, "", 0
    if cnt:
        out.append((first, lab, cnt, ""))
    return out


def table(mn):
    t = dict.fromkeys(CLASSES, 0)
    for m in mn:
        t[classify(m)] += 1
    return t


def main():
    args = [a for a in sys.argv[1:] if a != "--blocks"]
    path, subs = args[0], args[1:]
    if "--blocks" in sys.argv:
        for name, mn in kernels(path, labels=True):
            if not any(s in name for s in subs):
                continue
            print(name)
            print("  %6s %-12s %6s  %s" % ("first", "label", "count", "ends"))
            for first, lab, cnt, end in blocks(mn):
                print("  %6d %-12s %6d  %s" % (first, lab, cnt, end))
        return
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
