#!/bin/bash
# GPU box: everything the round's DESIGN.md / profiles/ numbers come from, in one run.
# usage: scripts/collect_evidence.sh <tag> [out dir]      (writes <out dir>, default evidence/ev/; profile_round.sh writes its own)
set -u
TAG=${1:-rXX}
EV=${2:-evidence/ev}
mkdir -p $EV
scripts/profile_recon.sh ${TAG}_res 128 resident > $EV/recon_resident.log 2>&1
scripts/profile_recon.sh ${TAG}_res256 256 resident > $EV/recon_resident_256.log 2>&1
scripts/profile_recon.sh ${TAG}_plain 128 plain > $EV/recon_plain.log 2>&1
python scripts/conv_bench.py 128 i8 > $EV/conv_bench_i8.txt 2>&1
python scripts/conv_bench.py 128 > $EV/conv_bench_f32.txt 2>&1
scripts/profile_conv_pmc.sh ${TAG}_l2 256 14 256 3 1 1 i8 > $EV/conv_pmc_256_14_256_3x3.txt 2>&1
scripts/profile_conv_pmc.sh ${TAG}_l1 64 56 256 1 1 0 i8 > $EV/conv_pmc_64_56_256_1x1.txt 2>&1
mkdir -p scripts/_bin
[ -x scripts/_bin/l2_probe ] || /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -o scripts/_bin/l2_probe scripts/l2_probe.hip 2>/dev/null
[ -x scripts/_bin/hbm_read_probe ] || /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -o scripts/_bin/hbm_read_probe scripts/hbm_read_probe.hip 2>/dev/null
scripts/_bin/hbm_read_probe > $EV/hbm_read_probe.txt 2>&1
{ python scripts/microbench.py 128; python scripts/microbench.py 128 --real; python scripts/microbench.py 128 --single; python scripts/microbench.py 128 --rotate 6; } 2>&1 | grep -v amdgpu.ids > $EV/microbench.txt
for b in 256 128 32 16 1; do python scripts/recon_probe.py $b 30 resident graph 2>&1 | tail -2; done > $EV/recon_graph.txt
python scripts/per_channel_probe.py 8 128 --phases 2>&1 | tail -2 > $EV/per_channel.txt
scripts/profile_round.sh $TAG > $EV/profile_round.log 2>&1
python bench.py --full > $EV/bench.json 2> $EV/bench.err
tail -3 $EV/recon_graph.txt; tail -c 600 $EV/bench.json
