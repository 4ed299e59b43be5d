#!/bin/bash
# Compares the gfx950 code of two source trees kernel by kernel: every cm_kernels*.hip of either tree (or the files named)
# is compiled to assembly with the flags of cloud_merger_amd/build.py, the __hip_cuid_* lines (the only thing that differs
# between two compilations of one source) are dropped, and per kernel one line says whether the text is identical, or else
# whether instruction count, code length, VGPRs, SGPRs, scratch and LDS are the same, or what differs. Cross-compiles, needs
# no GPU.
#   usage: bash scripts/kernel_isa_diff.sh TREE_A TREE_B [cm_kernels_x.hip ...] > profiles/NAME_isa.txt
set -euo pipefail
[ $# -ge 2 ] || { echo "usage: $0 TREE_A TREE_B [file.hip ...]" >&2; exit 2; }
A=$(cd "$1" && pwd); B=$(cd "$2" && pwd); shift 2
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-command-line-argument --cuda-device-only -S"
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
if [ $# -gt 0 ]; then FILES="$*"; else
  FILES=$( (cd "$A/cloud_merger_amd/csrc" && ls cm_kernels*.hip; cd "$B/cloud_merger_amd/csrc" && ls cm_kernels*.hip) | sort -u)
fi
mkdir -p "$TMP/a" "$TMP/b"
for f in $FILES; do
  for side in a b; do
    [ $side = a ] && src="$A/cloud_merger_amd/csrc" || src="$B/cloud_merger_amd/csrc"
    [ -f "$src/$f" ] && $HIPCC $FLAGS -I "$src" "$src/$f" -o "$TMP/$side/${f%.hip}.s" &
  done
  wait
done
python3 - "$TMP" $FILES <<'EOF'
import os, re, subprocess, sys

def kernels(path):
    """name -> (text lines, figures) of every function of an assembly file (kernels, and device functions left out of line)."""
    out, name, body, info = {}, None, [], None

    def close():
        if name is not None and info is not None:
            info["instructions"] = sum(1 for l in body if re.match(r"^\t[a-z]", l))
            out[name] = (body, info)

    for line in open(path):
        if "__hip_cuid_" in line:
            continue
        m = re.match(r"^(\w+):\s*; @", line)
        if m:
            close()
            name, body, info = m.group(1), [], None
        elif name is not None and info is None:
            if line.startswith(".Lfunc_end"):
                info = {}
            else:
                body.append(line.rstrip())
        elif info is not None:
            m = re.match(r"^; (codeLenInByte|TotalNumSgprs|NumSgprs|NumVgprs|NumAgprs|ScratchSize|LDSByteSize)\s*[:=]\s*(\d+)", line)
            if m:
                info[m.group(1).replace("TotalNumSgprs", "NumSgprs")] = int(m.group(2))
    close()
    return out

def demangle(n):
    try:
        d = subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
    except OSError:
        d = n
    d = re.sub(r"\(anonymous namespace\)::", "", d)
    d = re.sub(r"^void ", "", d)
    return d.split("(")[0]

FIG = [("instructions", "instructions"), ("codeLenInByte", "code bytes"), ("NumVgprs", "vgpr"), ("NumAgprs", "agpr"),
       ("NumSgprs", "sgpr"), ("ScratchSize", "scratch"), ("LDSByteSize", "lds")]
tmp, files = sys.argv[1], sys.argv[2:]
n_same = n_equal = n_diff = 0
for f in files:
    print("== " + f)
    pa, pb = (os.path.join(tmp, s, f[:-4] + ".s") for s in "ab")
    if not (os.path.exists(pa) and os.path.exists(pb)):
        print("  only in tree " + ("A" if os.path.exists(pa) else "B"))
        continue
    ka, kb = kernels(pa), kernels(pb)
    for n in sorted(set(ka) | set(kb), key=demangle):
        d = demangle(n)
        if n not in ka or n not in kb:
            print("  %-44s only in tree %s" % (d, "A" if n in ka else "B")); n_diff += 1
            continue
        (ta, ia), (tb, ib) = ka[n], kb[n]
        figs = "  ".join("%s %d" % (lab, ib.get(k, 0)) for k, lab in FIG)
        if ta == tb and ia == ib:
            print("  %-44s identical text (%s)" % (d, figs)); n_same += 1
        elif all(ia.get(k) == ib.get(k) for k, _ in FIG):
            print("  %-44s same figures, text differs (%s)" % (d, figs)); n_equal += 1
        else:
            ch = "  ".join("%s %d -> %d" % (lab, ia.get(k, 0), ib.get(k, 0)) for k, lab in FIG if ia.get(k) != ib.get(k))
            print("  %-44s DIFFERS: %s" % (d, ch)); n_diff += 1
print("# %d kernels identical in text, %d with the same figures, %d that differ" % (n_same, n_equal, n_diff))
EOF
