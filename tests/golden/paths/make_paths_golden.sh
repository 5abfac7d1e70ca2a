#!/bin/bash
# Regenerates tests/golden/paths/*.txt.gz: the trajectory files that the REFERENCE's own code writes for the .par files next to this script.
# Build machine only (it needs the reference's source tree: REF, default /root/reference).  Into a scratch directory it compiles, from the reference
# sources where they lie, the reference's trace_rays and trace_rays_imageplane programs (g++ -O2 -fopenmp -ffp-contract=off)
# and ref_paths_dump.cpp of this directory against the reference's classes (the RK4 write paths: the programs hard-wire Euler).
# Only the .par files and the outputs (gzip -n -9, so that the same text gives the same bytes) are fixtures; nothing of the reference's text is copied here.
#   ps_*.par  -> trace_rays            ip_*.par -> trace_rays_imageplane            rk4_*.par -> ref_paths_dump
# Every .par names `outfile = out.txt`: the programs run in a scratch directory and the file is compressed into <name>.txt.gz here.
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${REF:-/root/reference}
R=$REF/src
F="-O2 -fopenmp -ffp-contract=off -I$R -I$R/raytracer"
W=$(mktemp -d)
trap 'rm -rf "$W"' EXIT
( cd "$W" && g++ $F -c "$R/raytracer/raytracer.cpp" "$R/raytracer/pointsource.cpp" "$R/raytracer/imageplane.cpp" \
  && g++ $F "$R/ray_paths/trace_rays.cpp" raytracer.o pointsource.o -o trace_rays \
  && g++ $F "$R/ray_paths/trace_rays_imageplane.cpp" raytracer.o imageplane.o -o trace_rays_imageplane \
  && g++ $F "$HERE/ref_paths_dump.cpp" raytracer.o pointsource.o -o ref_paths_dump )
mkdir -p "$W/par" "$W/run"
for par in "$HERE"/*.par; do
    name=$(basename "$par" .par)
    rm -f "$W/run/out.txt" "$W/run/records.txt"
    case "$name" in
        # trace_rays keeps a pointer into a std::string that has gone out of scope when --parfile is given (trace_rays.cpp:27-31): it is run
        # where its built-in default ../par/trace_rays.par resolves
        ps_*)  cp "$par" "$W/par/trace_rays.par"; ( cd "$W/run" && ../trace_rays > /dev/null ) ;;
        ip_*)  ( cd "$W/run" && ../trace_rays_imageplane "$par" > /dev/null ) ;;
        rk4_*) ( cd "$W/run" && ../ref_paths_dump "$par" > /dev/null ) ;;
        *) echo "unknown case $name" >&2; exit 1 ;;
    esac
    gzip -n -9 -c "$W/run/out.txt" > "$HERE/$name.txt.gz"
    if [ -f "$W/run/records.txt" ]; then gzip -n -9 -c "$W/run/records.txt" > "$HERE/$name.records.txt.gz"; fi      # (records = 1: ref_paths_dump.cpp)
done
for f in "$HERE"/*.txt.gz; do echo "$f $(gzip -dc "$f" | wc -lc)"; done
