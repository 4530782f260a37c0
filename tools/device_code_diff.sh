#!/bin/bash
# Compare the gfx950 device code of two builds of libcone_hip.so kernel by kernel:
#   tools/device_code_diff.sh OTHER/cone_amd/libcone_hip.so [cone_amd/libcone_hip.so]
# Every code object of the .hip_fatbin section is extracted with the ROCm install's own tools and disassembled; the two
# disassemblies are split per symbol and compared as text, the kernel metadata notes (arguments, registers, LDS) as a
# whole.  Prints the symbols that differ or that only one library has, and exits 1 if there are any: a host-only
# change must leave this empty.
set -euo pipefail
A=$(readlink -f "$1"); B=$(readlink -f "${2:-$(dirname "$0")/../cone_amd/libcone_hip.so}")
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
dis() {     # library -> $2/NNN.s, one file per code object, in section order
    mkdir -p "$2"
    "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$1" "$2/fatbin"
    python3 - "$2" <<'EOF'
import struct, sys
d = sys.argv[1]
blob = open(d + "/fatbin", "rb").read()
magic = b"__CLANG_OFFLOAD_BUNDLE__"
pos, n = 0, 0
while True:
    pos = blob.find(magic, pos)
    if pos < 0:
        break
    cnt, = struct.unpack_from("<Q", blob, pos + 24)
    cur = pos + 32
    for _ in range(cnt):
        off, size, tl = struct.unpack_from("<QQQ", blob, cur)
        triple = blob[cur + 24:cur + 24 + tl].decode()
        cur += 24 + tl
        if "gfx950" in triple and size:
            open("%s/%03d.co" % (d, n), "wb").write(blob[pos + off:pos + off + size])
            n += 1
    pos += 24
EOF
    for co in "$2"/*.co; do
        "$LLVM/llvm-objdump" -d --no-show-raw-insn --no-leading-addr "$co" | grep -v 'file format' > "${co%.co}.s"
        "$LLVM/llvm-readelf" --notes "$co" | grep -v '^File:' > "${co%.co}.notes"      # kernel metadata: arguments, registers, LDS
    done
}
dis "$A" "$T/a"; dis "$B" "$T/b"
python3 - "$T/a" "$T/b" <<'EOF'
import glob, re, sys
def symbols(d):
    out = {}
    for f in sorted(glob.glob(d + "/*.s")):
        name = None
        for line in open(f):
            m = re.match(r"^<(.+)>:$", line.strip())
            if m:
                name = m.group(1); out[name] = []
            elif name:
                out[name].append(re.sub(r"\s*//.*$", "", line.rstrip()))   # (objdump's address comments are not code)
    return out
a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
notes = lambda d: [open(f).read() for f in sorted(glob.glob(d + "/*.notes"))]
if notes(sys.argv[1]) != notes(sys.argv[2]):
    bad.append("(kernel metadata notes)")
for k in bad:
    print(k if k.startswith("(") else ("only in first: " if k not in b else "only in second: " if k not in a else "differs: ") + k)
print("%d symbols in the first library, %d in the second, %d differ" % (len(a), len(b), len(bad)))
sys.exit(1 if bad else 0)
EOF
