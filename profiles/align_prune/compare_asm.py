"""Compare the gfx950 kernels of two builds of libmoni_hip.so instruction for instruction.

    python profiles/align_prune/compare_asm.py PARENT.s CHANGE.s > profiles/align_prune/kernels.txt

The two files are the device assembly that hipcc keeps with --save-temps (the flags of capi.build_lib() otherwise).  A kernel of the change is matched
with the parent's kernel of the same demangled name; the parent's chain_plan_kernel<WT, LEVEL, OCC, 64, GEN> is chain_plan_kernel<WT, LEVEL, OCC, GEN>.
Compared: the instruction stream (comments dropped; block labels by their number inside the function; a called function by the hash of its own
stream, so a callee whose name changed with a template argument still counts as the same code) and every .amdhsa_ line of the kernel descriptor.
One line per kernel: name, instructions, VGPRs, SGPRs, LDS bytes, scratch bytes, "identical" or how it differs from the parent's."""
import difflib
import hashlib
import re
import subprocess
import sys


def parse(path):
    """-> {symbol: [instruction lines]}, {kernel symbol: [.amdhsa_ lines]}"""
    funcs, desc = {}, {}
    cur = body = kd = None
    types = set()
    for raw in open(path):
        line = raw.split(";")[0].rstrip()
        s = line.strip()
        if not s:
            continue
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            types.add(m.group(1))
            continue
        if s.startswith(".amdhsa_kernel "):
            kd = desc.setdefault(s.split()[1], [])
            continue
        if s == ".end_amdhsa_kernel":
            kd = None
            continue
        if kd is not None:
            kd.append(s)
            continue
        if s.endswith(":") and s[:-1] in types and cur is None:
            cur, body = s[:-1], []
            continue
        if cur is not None:
            if s.startswith(".Lfunc_end"):
                funcs[cur] = body
                cur = None
            elif s.startswith(".L") and s.endswith(":"):
                body.append(re.sub(r"^\.L(\w+?)\d+_(\d+):", r".L\1_\2:", s))
            elif not s.startswith("."):
                body.append(s)
    return funcs, desc


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


class Build:
    def __init__(self, path):
        self.funcs, self.desc = parse(path)
        self.memo = {}

    def norm(self, sym, depth=0):
        """the function's stream with labels and symbols made comparable"""
        out = []
        for s in self.funcs[sym]:
            s = re.sub(r"\.L(BB|JTI|tmp)\d+_(\d+)", r".L\1_\2", s)
            s = re.sub(r"_Z\w+", lambda m: self.token(m.group(0), depth), s)
            out.append(s)
        return out

    def token(self, sym, depth):
        if sym in self.funcs and depth < 8:
            if sym not in self.memo:
                self.memo[sym] = "FN" + hashlib.sha1("\n".join(self.norm(sym, depth + 1)).encode()).hexdigest()[:12]
            return self.memo[sym]
        return "SYM"

    def resources(self, sym):
        d = dict(x.split(None, 1) for x in self.desc[sym])
        return tuple(d.get(k, "?") for k in (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size"))

    def descriptor(self, sym):
        return [re.sub(r"_Z\w+", lambda m: self.token(m.group(0).split(".")[0], 0), x) for x in self.desc[sym]]


def blank(x):
    return re.sub(r"\.L\w+", ".L", re.sub(r"\b([vsa])\d+\b", r"\1", re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[]", x)))


def short(name):          # (rocPRIM's kernels have names of a thousand characters)
    return name if len(name) <= 150 else name[:150] + "...#" + hashlib.sha1(name.encode()).hexdigest()[:6]


def key(name):
    return re.sub(r"(chain_plan_kernel<.*, \d, \d), 64, (true|false)>", r"\1, \2>", name)


def main():
    P, C = Build(sys.argv[1]), Build(sys.argv[2])
    dn_p, dn_c = demangle(sorted(P.desc)), demangle(sorted(C.desc))
    by_key = {key(dn_p[s]): s for s in P.desc}
    n_same = n_diff = 0
    seen = set()
    for s in sorted(C.desc, key=lambda x: dn_c[x]):
        name = dn_c[s]
        ins = C.norm(s)
        res = "%d instructions, VGPRs %s, SGPRs %s, LDS %s, scratch %s" % ((len([x for x in ins if not x.endswith(":")]),) + C.resources(s))
        p = by_key.get(name)
        if p is None:
            print("%s: %s: NEW (no kernel of this name in the parent)" % (short(name), res))
            n_diff += 1
            continue
        seen.add(p)
        pin = P.norm(p)
        verdict = "identical"
        if pin != ins:          # how far apart: the streams with register numbers and label numbers blanked, line by line
            bp, bc = [blank(x) for x in pin], [blank(x) for x in ins]
            ops = [o for o in difflib.SequenceMatcher(None, bp, bc, autojunk=False).get_opcodes() if o[0] != "equal"]
            verdict = "DIFFERENT: parent %d instructions, VGPRs %s, SGPRs %s, LDS %s, scratch %s; with register and label numbers blanked %d lines of the parent and %d of the change differ: %s" % (
                (len([x for x in pin if not x.endswith(":")]),) + P.resources(p) + (sum(o[2] - o[1] for o in ops), sum(o[4] - o[3] for o in ops),
                 " | ".join("%s -> %s" % ("; ".join(bp[o[1]:o[2]]) or "-", "; ".join(bc[o[3]:o[4]]) or "-") for o in ops[:12])))
        elif P.descriptor(p) != C.descriptor(s):
            verdict = "DIFFERENT descriptor: " + "; ".join("%s -> %s" % (a, b) for a, b in zip(P.descriptor(p), C.descriptor(s)) if a != b)
        n_same += verdict == "identical"
        n_diff += verdict != "identical"
        print("%s: %s: %s" % (short(name), res, verdict[:1500]))
    gone = sorted(dn_p[s] for s in P.desc if s not in seen)
    print("\n%d kernels identical, %d different or new; %d kernels of the parent are not in the change:" % (n_same, n_diff, len(gone)))
    for g in gone:
        print("  removed: " + g)


if __name__ == "__main__":
    main()
