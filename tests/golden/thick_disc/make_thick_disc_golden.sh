#!/bin/bash
# Regenerates tests/golden/thick_disc/*.txt.gz: what the REFERENCE's own integrators give for a finite-thickness disc handed to them as a user-defined
# RayDestination (ref_thick_dump.cpp of this directory has the subclass and the file formats).
# Build machine only (it needs the reference's source tree: REF, default /root/reference).  Into a scratch directory it compiles, from the reference
# sources where they lie, the reference's Raytracer and PointSource (g++ -O2 -fopenmp -ffp-contract=off) and ref_thick_dump.cpp
# against them.  Only the .par files and the outputs (gzip -n -9, so that the same text gives the same bytes) are fixtures; nothing of the reference's
# text is copied here.
#   rk4_*.par, rk45_*.par -> ref_thick_dump trace  -> <name>.records.txt.gz  (and <name>.init.txt.gz where the .par says init = 1)
#   probes_*.par          -> ref_thick_dump probes -> <name>.txt.gz
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${REF:-/root/reference}
R=$REF/src
F="-O2 -fopenmp -ffp-contract=off -I$R -I$R/raytracer"
W=$(mktemp -d)
trap 'rm -rf "$W"' EXIT
( cd "$W" && g++ $F -c "$R/raytracer/raytracer.cpp" "$R/raytracer/pointsource.cpp" \
  && g++ $F "$HERE/ref_thick_dump.cpp" raytracer.o pointsource.o -o ref_thick_dump )
mkdir -p "$W/run"
for par in "$HERE"/*.par; do
    name=$(basename "$par" .par)
    rm -f "$W/run/records.txt" "$W/run/init.txt" "$W/run/probes.txt"
    case "$name" in
        rk4_*|rk45_*) ( cd "$W/run" && ../ref_thick_dump trace "$par" > /dev/null )
                      gzip -n -9 -c "$W/run/records.txt" > "$HERE/$name.records.txt.gz"
                      if [ -f "$W/run/init.txt" ]; then gzip -n -9 -c "$W/run/init.txt" > "$HERE/$name.init.txt.gz"; fi ;;
        probes_*)     ( cd "$W/run" && ../ref_thick_dump probes "$par" > /dev/null )
                      gzip -n -9 -c "$W/run/probes.txt" > "$HERE/$name.txt.gz" ;;
        *) echo "unknown case $name" >&2; exit 1 ;;
    esac
done
for f in "$HERE"/*.txt.gz; do echo "$f $(gzip -dc "$f" | wc -lc) $(stat -c %s "$f")"; done
