#!/bin/bash
# A/B of the six image-plane disc programs (apps/imageplane_app.h) on their golden parameter files: another build of the programs, usually the
# parent commit's sources compiled against this tree's libkrtrace.so, twice (A1, A2), against this tree's apps/_build (B).
#   scripts/imageplane_apps_ab.sh <directory of the other build's programs> [output directory, default build/imageplane_apps_ab]
# then scripts/imageplane_apps_ab.py [output directory] compares what they wrote.  Every run has its own time limit; the first failure ends the script.
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
G=$ROOT/tests/golden/apps
OTHER=$(cd "$1" && pwd)
O=${2:-$ROOT/build/imageplane_apps_ab}
mkdir -p "$O" && O=$(cd "$O" && pwd)
run() {   # run <label> <bin dir> <case> <program> <ext> <args...>
    local label=$1 bin=$2 name=$3 prog=$4 ext=$5; shift 5
    local d=$O/$label; mkdir -p "$d"
    ( cd "$d" && timeout -k 10 120 "$bin/$prog" "$@" --outfile=$name.$ext --timing > $name.stdout 2> $name.stderr )
    local rc=$?
    echo "$label $name rc=$rc"
    if [ $rc -ne 0 ]; then tail -5 "$d/$name.stderr"; exit 1; fi
}
for pass in A1:$OTHER A2:$OTHER B:$ROOT/raytrace_cpu_amd/apps/_build; do
    L=${pass%%:*}; B=${pass#*:}
    run $L $B image_rk4 kr_imageplane_disc_image fits --parfile=$G/imageplane_rk4.par
    run $L $B image_rk45 kr_imageplane_disc_image fits --parfile=$G/imageplane_rk45.par
    run $L $B orders kr_imageplane_orders fits --parfile=$G/imageplane_orders.par
    run $L $B polarisation kr_imageplane_polarisation fits --parfile=$G/imageplane_polarisation.par --spec_outfile=polarisation_spec.dat
    run $L $B spectrum_thermal kr_disc_spectrum dat --parfile=$G/disc_spectrum_thermal.par
    run $L $B spectrum_table kr_disc_spectrum dat --parfile=$G/disc_spectrum_table.par --spec_file=$G/powerlaw.spec,$G/powerlaw.spec
    run $L $B hotspot kr_hotspot_lightcurve dat --parfile=$G/hotspot_lightcurve.par
    run $L $B line_rays kr_line_profile dat --parfile=$G/imageplane_rk4.par --line_mode=rays
    run $L $B line_pixels kr_line_profile dat --parfile=$G/imageplane_rk4.par --line_mode=pixels
done
echo "A/B runs complete"
