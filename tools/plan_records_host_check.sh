#!/bin/bash
# Host soundness of the plan's record handling under AddressSanitizer + UBSan (host code only, no GPU):
#   bash tools/plan_records_host_check.sh [build dir]
# builds the library's objects with the host sanitizers in a scratch copy of csrc/, links tools/plan_records_host_check.cpp against
# them, replays tests/golden/plan_calls.txt and compares the entry infos it prints with tests/golden/plan_entry_info.json.
set -euo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
dir=${1:-$(mktemp -d)}
san="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
mkdir -p "$dir/mindpose_amd" "$dir/tools"
mkdir -p "$dir/include" "$dir/mindpose_amd/csrc"
cp -u "$root"/include/*.h "$dir/include/"   # sources only (-u: a second run into the same directory rebuilds what changed)
cp -u "$root"/mindpose_amd/csrc/*.hip "$root"/mindpose_amd/csrc/*.h "$root"/mindpose_amd/csrc/Makefile "$dir/mindpose_amd/csrc/"
cp "$root/tools/plan_records_host_check.cpp" "$dir/tools/"
make -C "$dir/mindpose_amd/csrc" -j"${JOBS:-8}" EXTRA="$san -g" LIB=libmindpose_hip_san.so > "$dir/build.log" 2>&1 || { tail -30 "$dir/build.log"; exit 1; }
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
# the program itself is plain C++ (hipcc would compile a .cpp for the device too)
"$(dirname "$hipcc")/../lib/llvm/bin/clang++" -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -c "$dir/tools/plan_records_host_check.cpp" -o "$dir/tools/plan_records_host_check.o"
$hipcc --offload-arch=gfx950 -fsanitize=address,undefined "$dir/tools/plan_records_host_check.o" "$dir"/mindpose_amd/csrc/*.o -ldl \
    -o "$dir/plan_records_host_check"
"$dir/plan_records_host_check" "$root/tests/golden/plan_calls.txt" > "$dir/replay.txt"
tail -1 "$dir/replay.txt"
python3 - "$dir/replay.txt" "$root/tests/golden/plan_entry_info.json" <<'PY'
import json, sys
got = [[int(v) for v in line.split(":")[1].split()] for line in open(sys.argv[1]) if line.startswith("entry ")]
want = json.load(open(sys.argv[2]))
assert got == want["entries"], "entry infos differ from the fixture"
rcs = [int(line.split()[2]) for line in open(sys.argv[1]) if " rc " in line]
assert rcs == [c[1] for c in want["calls"]], "return codes differ from the fixture"
print(f"sanitizer replay clean: {len(rcs)} calls, {len(got)} entries match the fixture")
PY
