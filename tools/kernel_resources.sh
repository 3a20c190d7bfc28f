#!/bin/bash
# Development: VGPRs / scratch / occupancy and the scratch instructions on the loops of a few solve-kernel instantiations, in seconds and
# without a GPU - what a change to a rare block does to the allocation of the common paths (the certificate experiments of round 5:
# profiles/r50_kernel_resources.log).      bash tools/kernel_resources.sh [csrc directory] [tag]
#                                          bash tools/kernel_resources.sh simplex [csrc directory] [tag]      the in-wave simplex kernels instead
src=${1:-$(cd "$(dirname "$0")/../dispatches_amd/csrc" && pwd)}; tag=${2:-cur}; out=${TMPDIR:-/tmp}/kres; mkdir -p $out
if [ "$1" = simplex ]; then
  # every instantiation of csrc/dsp_simplex.hip (plain and CERT: dsp_options::simplex_certify), dynamic LDS from simplex_lds_bytes at its shape
  src=${2:-$(cd "$(dirname "$0")/../dispatches_amd/csrc" && pwd)}; tag=${3:-cur}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 $KRES_FLAGS -S --cuda-device-only -I$src -o $out/$tag.simplex.s $src/dsp_simplex.hip -Rpass-analysis=kernel-resource-usage 2> $out/$tag.simplex.res
  python - $out/$tag.simplex.res <<'PY'
import re, sys
lds = lambda n, m: (m * ((n + m) | 1) + 2 * ((m + 1) & ~1) + ((n + m + 1) & ~1) + 16) * 8      # simplex_lds_bytes
for blk in open(sys.argv[1]).read().split("Function Name: ")[1:]:
    name = re.search(r"simplex_\w*?kernelI\w+?EE", blk.split("\n")[0]).group(0)
    g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
    args = [int(v) for v in re.findall(r"L[ib](\d+)E", name)]
    kind = "reg" if "reg" in name else "lds"
    label = f"simplex_{'reg_' if kind == 'reg' else ''}kernel<{', '.join(str(v) for v in args)}>"
    dyn = "static 1024 B" if kind == "reg" else (f"dynamic, {lds(34, 20)} B at 34 x 20 (4-h wind + battery)" if args[0] == 1 else f"dynamic, {lds(64, 64)} B at 64 x 64")
    scr, occ = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]")
    print(f"{label:32s} VGPRs {g('VGPRs')} AGPRs {g('AGPRs')} scratch {scr:4d} B/lane occupancy {occ} LDS {dyn}")
PY
  exit 0
fi
cat > $out/$tag.hip <<EOT
#define DSP_KERNELS_ONLY
#include "$src/dsp_kernels.hip"
namespace dsp {
template __global__ void pdlp_solve_kernel<4, 2, false, 0x1133u, 0x44u, false>(SolveArgs);           // wind + battery 24 h (metric)
template __global__ void pdlp_solve_kernel<7, 4, false, 0x1112333u, 0x2444u, false>(SolveArgs);      // wind + battery 48 h
template __global__ void pdlp_solve_kernel<4, 3, true, 0x1122u, 0x233u, false>(SolveArgs);           // wind + PEM 48 h
template __global__ void pdlp_solve_kernel<3, 2, false, 0x122u, 0x24u, false>(SolveArgs);            // nuclear 24 h
template __global__ void pdlp_solve_kernel<1, 1, false, 0x3u, 0x4u, false>(SolveArgs);               // 4-h hourly LPs
template __global__ void pdlp_solve_kernel<4, 2, false, 0u, 0u, false>(SolveArgs);                   // generic (LDS matrix, with certificates)
$(grep -q 'bool LIGHT' "$src/dsp_kernels.hip" && echo 'template __global__ void pdlp_solve_kernel<4, 2, false, 0u, 0u, false, true>(SolveArgs);             // ... its light instantiation (follow-up passes of a three-wave first pass)')
}
EOT
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 $KRES_FLAGS -S --cuda-device-only -I$src -o $out/$tag.s $out/$tag.hip -Rpass-analysis=kernel-resource-usage 2> $out/$tag.res
python - $out/$tag.s $out/$tag.res <<'PY'
import re, sys
src = open(sys.argv[1]).read(); res = open(sys.argv[2]).read()
for blk in res.split("Function Name: ")[1:]:
    name = blk.split("\n")[0].split(" [")[0].strip()
    if "pdlp_solve" not in name: continue
    g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
    i = src.index("\n" + name + ":"); body = src[i:src.index(".Lfunc_end", i)].split("\n")
    labels = {m.group(1): k for k, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    loops = []
    for k, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l) or re.search(r"s_branch (\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < k:
            seg = body[labels[m.group(1)]:k + 1]
            loops.append((len(seg), sum("v_fma_f64" in s for s in seg), sum("scratch_" in s for s in seg)))
    loops = sorted(L for L in loops if L[1] >= 8)[:3]
    scr, occ = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]")
    print(f"{name[28:62]:36s} VGPRs {g('VGPRs')} scratch {scr:4d} B/lane occupancy {occ} | scratch instructions {sum('scratch_' in s for s in body):4d} "
          f"| innermost loops (lines, FMAs, scratch instructions) {loops}")
PY
