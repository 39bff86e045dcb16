"""CPU (hipcc cross-compiles without a GPU): registers and scratch of the fp32 EM sweep for index records
(msweep_amd/csrc/em_f32_kernels.hpp k_em_passB_f32_idx), both slice-class instantiations, in a translation unit of their
own like tests/test_kernel_resources.py.  The kernel is launched with 1024 threads -- 16 wavefronts on 4 SIMDs of 512
registers -- so 128 registers per lane is the ceiling, and a spill (which no parity test sees) would drain the record
prefetch in every slice: zero scratch."""
import os

from kernel_resources import compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "kernels.hpp"
#include "em_kernels.hpp"
#include "em_f32_kernels.hpp"
using namespace msw;
template __global__ void msw::k_em_passB_f32_idx<false>(const Scalars *, SellDev, const double *, const float *, const float *, double *, double *, GuardDev);
template __global__ void msw::k_em_passB_f32_idx<true>(const Scalars *, SellDev, const double *, const float *, const float *, double *, double *, GuardDev);
'''
LIMITS = [("k_em_passB_f32_idxILb0E", 128), ("k_em_passB_f32_idxILb1E", 128)]


def test_index_float_sweep_fits_its_registers_without_scratch(tmp_path):
    res = compile_resources(TU, tmp_path, "mini")
    for frag, vmax in LIMITS:
        hit = [(k, v) for k, v in res.items() if frag in k]
        assert len(hit) == 1, (frag, [k for k in res if "k_em" in k])
        name, v = hit[0]
        print(name, v)
        assert v["ScratchSize"] == 0, f"{frag}: {v['ScratchSize']} bytes of scratch per lane"
        assert v["VGPRs"] <= vmax, f"{frag}: {v['VGPRs']} registers (ceiling {vmax})"
        # the sweeps' LDS image starts at LDS address 0: no static LDS of the kernel's own (sweep_launch.hpp prepare_sweep)
        assert v["LDS Size"] == 0, f"{frag}: {v['LDS Size']} bytes of static LDS"
