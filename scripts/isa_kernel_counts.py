"""Per-kernel instruction counts of gfx950 listings (hipcc -S --cuda-device-only): prints JSON {listing: {symbol: [instructions, sha1]}}.

    python scripts/isa_kernel_counts.py a.s b.s > counts.json

A function runs from its `symbol:` label (a symbol with `.type symbol,@function`) to `.Lfunc_end`; an instruction is a line that is no
label, directive or comment.  The hash is over the instruction text, comments stripped, block labels without the function's number.  tests/test_experts_isa.py compares the library's
kernels with the record made from the commit before the expert sets (tests/golden/isa_kernels_before_experts.json)."""
import hashlib
import json
import os
import re
import sys


def kernel_counts(path):
    functions = set()
    lines = open(path).read().split("\n")
    for l in lines:
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", l)
        if m:
            functions.add(m.group(1))
    out, cur, n, h = {}, None, 0, None
    for l in lines:
        s = l.split(";")[0].strip()
        m = re.match(r"([\w.$]+):$", s)
        if m and m.group(1) in functions:
            cur, n, h = m.group(1), 0, hashlib.sha1()
            continue
        if cur is None or not s:
            continue
        if s.startswith(".Lfunc_end"):
            out[cur] = [n, h.hexdigest()]
            cur = None
            continue
        if s.startswith(".") or s.endswith(":"):
            continue
        n += 1
        h.update((re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())) + "\n").encode())     # (block labels carry the function's number in its file)
    return out


if __name__ == "__main__":
    print(json.dumps({os.path.basename(p): kernel_counts(p) for p in sys.argv[1:]}, indent=0, sort_keys=True))
