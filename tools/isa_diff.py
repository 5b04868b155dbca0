#!/usr/bin/env python
"""Which kernels changed between two builds?  Compares the instruction streams function by function (labels normalised,
comments and directives dropped) of two sets of device assembly files, e.g.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -munsafe-fp-atomics -S --cuda-device-only gemm_bf16.hip -o before.s
    ... edit: add a new template instantiation / constexpr branch ...
    hipcc ... -o after.s ;  python tools/isa_diff.py before.s after.s

Either side may be several files, separated by commas or by `--` (a translation unit that was split: gemm_bf16.hip,
gemm_bf16_pack.hip, gemm_bf16_wgrad.hip):   python tools/isa_diff.py before.s -- fwd.s pack.s wgrad.s
A kernel whose mangled name is gone while a new name carries the identical stream (its template parameters changed) is reported
RENAMED and does not count as a change.

Used to add experimental kernel variants as NEW instantiations, and to refactor host code, while proving that every validated
kernel is unchanged instruction for instruction (no GPU needed).  Exit status 1 if any kernel CHANGED."""
import re
import sys


def norm(t):
    """label numbers count up through a translation unit: .LBB<function>_<block>, and .Lpost_getpc<n> of a long branch"""
    return re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", t))


def funcs(paths):
    out, cur = {}, None
    for line in (ln for path in paths for ln in open(path)):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.strip().startswith(".end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = re.sub(r";.*", "", line).strip()
        if t and not t.startswith("."):
            out[cur].append(norm(t))
        elif t.startswith(".LBB"):
            out[cur].append(norm(t))
    return out


def main(a_paths, b_paths):
    a, b = funcs(a_paths), funcs(b_paths)
    changed = [k for k in a if k in b and a[k] != b[k]]
    for k in changed:
        print(f"CHANGED  {k[:110]}  ({len(a[k])} -> {len(b[k])} instructions)")
    removed = [k for k in a if k not in b]
    renamed = 0
    for k in b:
        if k in a:
            continue
        old = next((r for r in removed if a[r] == b[k]), None)
        if old is None:
            print(f"NEW      {k[:110]}  ({len(b[k])} instructions)")
        else:
            removed.remove(old)
            renamed += 1
            print(f"RENAMED  {old[:110]}\n      -> {k[:110]}  ({len(b[k])} instructions)")
    for k in removed:
        print(f"REMOVED  {k[:110]}")
    print(f"{len(a)} -> {len(b)} kernels, {len(changed)} changed, {renamed} renamed")
    return 1 if changed else 0


def sides(argv):
    """[before..., '--', after...] or [before(,before...), after(,after...)]"""
    if "--" in argv:
        i = argv.index("--")
        return argv[:i], argv[i + 1:]
    if len(argv) != 2:
        raise SystemExit(__doc__)
    return argv[0].split(","), argv[1].split(",")


if __name__ == "__main__":
    sys.exit(main(*sides(sys.argv[1:])))
