#!/bin/bash
# Device code of two builds of libkvhip.so compared kernel by kernel (no GPU needed):
#   tools/kdiff.sh <parent libkvhip.so> <new libkvhip.so>
# Every gfx950 code object of each library is taken out of its fat binary; kernels are keyed by their demangled name with
# "(anonymous namespace)::" removed (a kernel header included by several units gives several copies of one name).  Reports:
# the totals, names lost or new, names whose copy count changed, names whose VGPR / SGPR / LDS / scratch / kernarg figures
# differ, and names with an instruction sequence in the new build that no copy in the parent has.  Exit status 1 if a name
# was lost or is new, a figure or a sequence differs, or the total rose.
set -e
exec python3 - "$1" "$2" <<'EOF'
import collections, hashlib, os, re, struct, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

def code_objects(lib):
    data = open(lib, "rb").read()
    out, at = [], data.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + 24)
        p = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size: out.append(data[at + off:at + off + size])
        at = data.find(MAGIC, at + 1)
    return out

def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    # (up to the parameter list, as tools/kres.sh prints it: template arguments tell the instantiations apart)
    return {m: d.replace("(anonymous namespace)::", "").replace("void ", "", 1).split("(")[0] for m, d in zip(names, r)}

def kernels(lib):
    """name -> list of (figures, hash of the instruction sequence, instruction count), one per copy"""
    found = collections.defaultdict(list)
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib)):
            path = os.path.join(tmp, "u%d.elf" % i)
            open(path, "wb").write(co)
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", path], capture_output=True, text=True).stdout
            figs = {}
            for block in re.split(r"\n\s+- \.agpr_count:|\n\s+- \.args:", notes):
                f = dict(re.findall(r"\.(\w+):\s+(\S+)", block))
                if "symbol" in f and "vgpr_count" in f:
                    figs[f["symbol"][:-3] if f["symbol"].endswith(".kd") else f["symbol"]] = tuple(
                        f.get(k, "?") for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size",
                                                "private_segment_fixed_size", "kernarg_segment_size"))
            dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True).stdout
            cur, seq = None, []
            def close():
                while seq and re.match(r"s_nop|s_code_end", seq[-1]): seq.pop()   # the padding behind a kernel
                if cur in figs:
                    found[cur].append((figs[cur], hashlib.sha1("\n".join(seq).encode()).hexdigest(), len(seq)))
            for line in dis.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    close()
                    cur, seq = m.group(1), []
                elif cur and line.startswith("\t") and line.strip() != "...":   # (... : the zero padding behind a kernel)
                    seq.append(re.sub(r"\s*//.*$", "", line).strip())
            close()
    dm = demangle(sorted(found))
    by = collections.defaultdict(list)
    for m, copies in found.items(): by[dm[m]].extend(copies)
    return by

a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
na, nb = sum(map(len, a.values())), sum(map(len, b.values()))
print("kernel symbols: parent %d, new %d; distinct names: parent %d, new %d" % (na, nb, len(a), len(b)))
bad = nb > na
for n in sorted(set(a) - set(b)): print("LOST  ", n); bad = True
for n in sorted(set(b) - set(a)): print("NEW   ", n); bad = True
for n in sorted(set(a) & set(b)):
    if len(a[n]) != len(b[n]): print("copies %d -> %d  %s" % (len(a[n]), len(b[n]), n))
for n in sorted(set(a) & set(b)):
    fa, fb = {c[0] for c in a[n]}, {c[0] for c in b[n]}
    if not fb <= fa: print("FIGURES (vgpr, sgpr, lds, scratch, kernarg) %s -> %s  %s" % (sorted(fa), sorted(fb), n)); bad = True
    ha = {c[1] for c in a[n]}
    for c in b[n]:
        if c[1] not in ha:
            print("CODE   %s: a sequence of %d instructions the parent has not (parent: %s)" % (n, c[2], sorted({x[2] for x in a[n]})))
            bad = True
sys.exit(1 if bad else 0)
EOF
