#!/bin/bash
# Regenerates tests/golden/healpix_vectors.npz: the pixel vectors of the REFERENCE's own healpix.h (get_pixel_vectors<double>) at all pixels of orders
# 0-3 and 512 sampled pixels each of orders 8 and 12 (healpix_vectors_dump.cpp of this directory says which).
# Build machine only (it needs the reference's source tree: REF, default /root/reference): the driver is compiled against the header where it lies,
# with the flags of the reference's own build (g++ -O2 -ffp-contract=off).  Only the recorded numbers are the fixture:
# order int32[n], pix int64[n], bits uint64[n][15] (the doubles' bit patterns: four corners then the centre).
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${REF:-/root/reference}
W=$(mktemp -d)
trap 'rm -rf "$W"' EXIT
g++ -O2 -ffp-contract=off -I"$REF/src/include" "$HERE/healpix_vectors_dump.cpp" -o "$W/dump"
"$W/dump" "$W/vectors.bin"
python3 - "$W/vectors.bin" "$HERE/healpix_vectors.npz" <<'EOF'
import sys
import numpy as np
rec = np.fromfile(sys.argv[1], dtype=np.dtype([("order", "<i4"), ("pix", "<i4"), ("bits", "<u8", 15)]))
np.savez_compressed(sys.argv[2], order=rec["order"].astype(np.int32), pix=rec["pix"].astype(np.int64), bits=np.ascontiguousarray(rec["bits"]))
print(sys.argv[2], len(rec), "pixels;", {int(o): int((rec["order"] == o).sum()) for o in np.unique(rec["order"])})
EOF
