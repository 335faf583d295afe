"""Compare the instruction stream of one kernel in two hipcc -S listings: python profiles/detect_fit_asmdiff.py OLD.s OLD_SYMBOL_PART
NEW.s NEW_SYMBOL_PART.  Labels are renumbered in order of appearance, comments and directives dropped; prints the number of
instructions on either side and a unified diff (empty: the same instructions)."""
import difflib
import re
import sys


def body(path, part):
    lines = open(path).read().splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_Z\S*:", ln) and part in ln.split(":")[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    names, out = {}, []

    def label(m):
        return names.setdefault(m.group(0), f".L{len(names)}")

    for ln in lines[start + 1:end]:
        ln = ln.split(";")[0].rstrip()
        if not ln.strip() or ln.strip().startswith((".p2align", ".section", ".type", ".size")):
            continue
        out.append(re.sub(r"\.LBB\d+_\d+", label, ln.strip()))
    return out


if __name__ == "__main__":
    a, b = body(sys.argv[1], sys.argv[2]), body(sys.argv[3], sys.argv[4])
    print(f"{len(a)} lines against {len(b)}")
    diff = list(difflib.unified_diff(a, b, lineterm="", n=1))
    print("\n".join(diff) if diff else "identical")
    sys.exit(1 if diff else 0)
