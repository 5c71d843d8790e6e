#!/bin/bash
# diagnostic build: the product's objects with dec_persist.hip (the one source that reads the macro) rebuilt under -DG2V_PSTAMPS
# -> libg2v_pstamps.so beside this script.  Further arguments go to that compile.
set -e
here="$(cd "$(dirname "$0")" && pwd)"
cd "$here/../gesture2vec_amd/csrc"
make -j4
obj="${TMPDIR:-/tmp}/pst"; mkdir -p "$obj"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -DG2V_PSTAMPS "$@" -c dec_persist.hip -o "$obj/dec_persist.o"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $(ls *.o | grep -v '^dec_persist\.o$') "$obj/dec_persist.o" -o "$here/libg2v_pstamps.so"
