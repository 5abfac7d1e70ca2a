#!/bin/bash
# Regenerates tests/golden/apps/caustic_plane_grid.fits: the output of the REFERENCE's own caustic_plane program (CPU build, oracle/_ref/apps/,
# produced by oracle/build_dropin_apps.sh from the reference sources) on caustic_plane_grid.par -- the par file of caustic_plane.par with
# bundle_eps_frac = 0, i.e. the grid-neighbour Jacobian.  Build container only; 0.3 s.  The fixture is the program's output file (data), nothing
# else.  Kept on RK4: the grid holds the pixel (0, 0), whose ray the reference's RK45 never returns from.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
APPS=$HERE/../../oracle/_ref/apps
G=$HERE/apps
export LD_PRELOAD=/usr/lib/x86_64-linux-gnu/libstdc++.so.6 LD_LIBRARY_PATH=/opt/conda/lib
rm -f $G/caustic_plane_grid.fits
$APPS/caustic_plane --parfile=$G/caustic_plane_grid.par --outfile=$G/caustic_plane_grid.fits > /dev/null
ls -la $G/caustic_plane_grid.*
