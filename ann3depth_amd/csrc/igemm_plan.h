// igemm_plan.h — what the tile / split-K planner (igemm_plan.cc) is asked and what it answers.  Plain C++: the planner
// runs on the host, inside the *_ws_bytes queries too, and needs nothing of HIP.
#pragma once
#include <stddef.h>

namespace a3d {

enum { MODE_FWD = 0, MODE_BWD_D = 1, MODE_BWD_F = 2 };

// Environment switches (capi.cc).  tune_int: A/B and sweep switches — the environment is consulted ONLY in a process started
// with A3D_TUNING=1 (the tools under tools/ set it); anywhere else the default is returned and nothing reads the environment.
bool tuning();
int tune_int(const char* name, int dflt);

struct GemmPlan {
  int prec;          // A3D_PREC_*: 0 = fp32 kernel (cfg valid), else bf16 kernel (bf16_bn valid)
  int bf16_bn;       // 128 or 64
  int cfg;           // index into kCfgs (igemm_cfgs.h)
  int splitk;
  int ktiles_per_split;
  int tiles_m, tiles_n;
  int streamk;       // > 0: stream-K launch of this many blocks (splitk == 1)
  size_t ws_bytes;   // split-K / stream-K slabs (0 if neither)
  int ring;          // bf16 plans: 1 + index into kRingCfgs of the LDS-DMA kernel for bf16-stored operands (igemm_ring.h), 0 = igemm_bf16
};

struct GemmProblem {
  int mode;          // MODE_*
  int M, N, K;
  int avec, bvec;    // 1 or 4
  int plain = 0;     // 1: register-staged kernel without split-K only (fused-pool forward)
  int need_reduce = 0;   // 1: the output is stored by the split-K reduction only (rows narrower than the GEMM's N): split-K >= 2, no stream-K
  int no_glds = 0;   // 1: not the LDS-DMA kernels (bf16 output)
  int ring_ok = 0;   // 1: both operands are bf16 tensors whose 16-byte pieces lie inside one filter tap (channels % 8 == 0):
                     //    forward / stride-1 bwd-data may run on igemm_ring.h
};

GemmPlan plan_gemm(const GemmProblem& g, int precision = 0);
// `pl` if its slabs (and `per_split` more bytes per split: the bias gradient's row) fit into `avail` workspace bytes, else the same
// tile with the deepest split-K that does, down to the unsplit launch, which needs none
GemmPlan plan_within(const GemmProblem& g, GemmPlan pl, size_t avail, size_t per_split);

}  // namespace a3d
