#!/bin/bash
# tools/copy_closing.sh <tag>: what tools/closing_run.sh left under gpurun_out/ into profiles/ (the tracked copies the design cites)
TAG=${1:-r04}
cd "$(dirname "$0")/.."
cp gpurun_out/prof_$TAG/summary.txt profiles/${TAG}_bench_longbackref_256x4MiB.txt
cp gpurun_out/prof_${TAG}_highentropy/summary.txt profiles/${TAG}_bench_highentropy_256x4MiB.txt
cp gpurun_out/prof_${TAG}_alice29x1024/summary.txt profiles/${TAG}_bench_alice29x1024.txt
cp gpurun_out/prof_$TAG/pmc.json profiles/pmc_$TAG.json
cp gpurun_out/prof_${TAG}_highentropy/pmc.json profiles/pmc_${TAG}_highentropy.json
cp gpurun_out/prof_${TAG}_alice29x1024/pmc.json profiles/pmc_${TAG}_alice29x1024.json
tail -1 gpurun_out/closing_$TAG/bench_default.json > profiles/${TAG}_bench_default.json
ls -la profiles | grep $TAG
