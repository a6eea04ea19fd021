// optim.hip — cmb_grad_sqnorm and cmb_adamw_step: the global gradient norm and a one-pass AdamW step over a TABLE of tensors.
//
// The reference trains under Hugging Face's default max_grad_norm = 1.0 (train_fsdp.py:122 derives its TrainingArguments from
// transformers', no script passes --max_grad_norm): a global L2 clip before every optimizer step.  cmb_grad_sqnorm forms
// sum g^2 over every gradient of the table; cmb_adamw_step reads that scalar ON THE DEVICE, folds the clip coefficient into
// the gradient scale and applies torch.optim.AdamW's update to the fp32 parameters (masters) and both moments in one pass,
// writing the bf16 compute copy of a master in the same pass — no host synchronisation, no scaled-gradient pass, no up-cast /
// cast-back passes.
//
// Both are HBM streaming kernels: a workgroup of 256 threads owns one chunk of CMB_OPTIM_CHUNK elements of one tensor at a
// time (its job found by bisection over the jobs' first-chunk prefix, as weight_prep does for tiles), the grid is capped and
// strides over the chunks, a thread moves 8 elements per round with 16-byte accesses.  A job whose pointers are not all
// 16-byte aligned (a view at an odd offset of a flat bucket) takes element-wise accesses instead; the choice is per job,
// hence uniform in the workgroup.  The sum is deterministic and independent of the grid and of the access path: a chunk's sum
// has a fixed order (optim_core.h) and goes to partial[chunk], a second one-wave launch adds the partials in index order in
// fp64.  No atomics, no completion counters.  All arithmetic is optim_core.h (host + device), run on the CPU by
// tests/csrc/optim_sim.cpp.
#include "common.h"
#include "optim_core.h"

namespace {

typedef uint16_t u16x8_t __attribute__((ext_vector_type(8)));
constexpr int kMaxGrid = 2048;   // 256 CUs x 8 workgroups of 256 threads

__device__ __forceinline__ bool al16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// the job that owns chunk c: the last one whose first chunk is <= c (empty jobs share their chunk0 with the next job and are
// never the last such one)
__device__ __forceinline__ cmb_optim_job find_job(const cmb_optim_job* __restrict__ jobs, int64_t n_jobs, int64_t c) {
  int64_t lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (jobs[mid].chunk0 <= c) lo = mid;
    else hi = mid - 1;
  }
  return jobs[lo];
}

// 8 gradient elements at p as floats: one 16-byte load (bf16) or two (fp32)
__device__ __forceinline__ void load8_grad(const void* g, int dtype, int64_t i, float (&x)[8]) {
  if (dtype == CMB_F32) {
    Vec8<float>::load(reinterpret_cast<const float*>(g) + i, x);
  } else {
    const u16x8_t h = *reinterpret_cast<const u16x8_t*>(reinterpret_cast<const uint16_t*>(g) + i);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = cmb_bf16_widen(h[e]);
  }
}
__device__ __forceinline__ float load1_grad(const void* g, int dtype, int64_t i) {
  return dtype == CMB_F32 ? reinterpret_cast<const float*>(g)[i] : cmb_bf16_widen(reinterpret_cast<const uint16_t*>(g)[i]);
}

// ---- sum of squares ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CMB_OPTIM_THREADS) grad_sqnorm_kernel(const cmb_optim_job* __restrict__ jobs,
                                                                        int64_t n_jobs, int64_t total_chunks,
                                                                        float* __restrict__ partial) {
  __shared__ float red[CMB_OPTIM_THREADS];
  const int tid = threadIdx.x;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    const cmb_optim_job j = find_job(jobs, n_jobs, c);
    const int64_t off = (c - j.chunk0) * CMB_OPTIM_CHUNK;
    const int64_t rest = j.n - off;
    const int n_left = rest < CMB_OPTIM_CHUNK ? (int)rest : CMB_OPTIM_CHUNK;
    const bool vec = al16(j.grad);   // (chunk offsets are multiples of 16 bytes)
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = tid * 8; base < n_left; base += CMB_OPTIM_ROUND) {
      float x[8];
      if (vec && base + 8 <= n_left) {
        load8_grad(j.grad, j.grad_dtype, off + base, x);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = base + e < n_left ? load1_grad(j.grad, j.grad_dtype, off + base + e) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) cmb_optim_sq_accum(acc[e], x[e]);
    }
    red[tid] = cmb_optim_sum8(acc);
    __syncthreads();
    for (int o = CMB_OPTIM_THREADS / 2; o > 0; o >>= 1) {
      cmb_optim_tree_lane(red, tid, o);
      __syncthreads();
    }
    if (tid == 0) partial[c] = red[0];
  }
}

// one wave: lane l loads partial[b * 64 + l], the 64 values are added in index order (every lane forms the same sum)
__global__ void __launch_bounds__(64) grad_sqnorm_final_kernel(const float* __restrict__ partial, int64_t n,
                                                               float* __restrict__ out) {
  const int lane = threadIdx.x;
  double s = 0.0;
  float next = lane < n ? partial[lane] : 0.f;
  for (int64_t b = 0; b < n; b += 64) {
    const float cur = next;
    const int64_t nb = b + 64 + lane;
    next = nb < n ? partial[nb] : 0.f;   // (a padding +0 leaves the sum unchanged)
#pragma unroll
    for (int k = 0; k < 64; ++k) s = cmb_optim_final_add(s, __shfl(cur, k, 64));
  }
  if (lane == 0) out[0] = (float)s;
}

// ---- AdamW --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store8_low(uint16_t* low, int64_t i, const float (&p)[8]) {
  u16x8_t h;
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = cmb_bf16_rne(p[e]);
  *reinterpret_cast<u16x8_t*>(low + i) = h;
}

__global__ void __launch_bounds__(CMB_OPTIM_THREADS) adamw_step_kernel(const cmb_optim_job* __restrict__ jobs, int64_t n_jobs,
                                                                       int64_t total_chunks, const cmb_adamw_consts k,
                                                                       float grad_scale, const float* __restrict__ sumsq,
                                                                       float max_norm) {
  const int tid = threadIdx.x;
  // the clip coefficient comes from device memory: every workgroup evaluates the same expression on the same scalar
  const float gs = sumsq ? grad_scale * cmb_optim_clip_coef(sumsq[0], grad_scale, max_norm) : grad_scale;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    const cmb_optim_job j = find_job(jobs, n_jobs, c);
    const int64_t off = (c - j.chunk0) * CMB_OPTIM_CHUNK;
    const int64_t rest = j.n - off;
    const int n_left = rest < CMB_OPTIM_CHUNK ? (int)rest : CMB_OPTIM_CHUNK;
    float* __restrict__ P = j.param + off;
    float* __restrict__ M = j.exp_avg + off;
    float* __restrict__ V = j.exp_avg_sq + off;
    uint16_t* __restrict__ LOW = j.low ? reinterpret_cast<uint16_t*>(j.low) + off : nullptr;
    const bool vec = al16(j.grad) && al16(j.param) && al16(j.low) && al16(j.exp_avg) && al16(j.exp_avg_sq);
    const int n_vec = vec ? (n_left & ~7) : 0;   // whole 8-element vectors; the rest goes one element at a time
    for (int base = tid * 8; base < n_vec; base += CMB_OPTIM_ROUND) {
      float g[8], p[8], m[8], v[8];
      load8_grad(j.grad, j.grad_dtype, off + base, g);
      Vec8<float>::load(P + base, p);
      Vec8<float>::load(M + base, m);
      Vec8<float>::load(V + base, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) cmb_adamw_update(g[e] * gs, p[e], m[e], v[e], k);
      Vec8<float>::store(P + base, p);
      Vec8<float>::store(M + base, m);
      Vec8<float>::store(V + base, v);
      if (LOW) store8_low(LOW, base, p);
    }
    for (int i = n_vec + tid; i < n_left; i += CMB_OPTIM_THREADS) {
      float p = P[i], m = M[i], v = V[i];
      cmb_adamw_update(load1_grad(j.grad, j.grad_dtype, off + i) * gs, p, m, v, k);
      P[i] = p;
      M[i] = m;
      V[i] = v;
      if (LOW) LOW[i] = cmb_bf16_rne(p);
    }
  }
}

int check_table(const cmb_optim_job* jobs, int64_t n_jobs, int64_t total_chunks) {
  if (n_jobs < 0 || total_chunks < 0) return CMB_ERR_BAD_ARG;
  if (n_jobs > 0 && !jobs) return CMB_ERR_BAD_ARG;
  if (n_jobs == 0 && total_chunks > 0) return CMB_ERR_BAD_ARG;   // chunks of no tensor
  return CMB_OK;
}

unsigned grid_for(int64_t total_chunks) { return (unsigned)(total_chunks < kMaxGrid ? total_chunks : kMaxGrid); }

}  // namespace

extern "C" int64_t cmb_optim_chunks(int64_t n) { return cmb_optim_chunks_of(n); }

extern "C" int64_t cmb_grad_sqnorm_workspace(int64_t total_chunks) { return total_chunks > 0 ? total_chunks : 0; }

extern "C" int cmb_grad_sqnorm(const cmb_optim_job* jobs_device, int64_t n_jobs, int64_t total_chunks, float* partial,
                               int64_t partial_floats, float* sumsq_out, void* stream) {
  const int rc = check_table(jobs_device, n_jobs, total_chunks);
  if (rc != CMB_OK) return rc;
  if (!sumsq_out || partial_floats < 0 || (total_chunks > 0 && !partial)) return CMB_ERR_BAD_ARG;
  if (partial_floats < cmb_grad_sqnorm_workspace(total_chunks)) return CMB_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (total_chunks > 0) {
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid_for(total_chunks)), dim3(CMB_OPTIM_THREADS), 0, s, jobs_device, n_jobs,
                       total_chunks, partial);
    CMB_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(64), 0, s, (const float*)partial, total_chunks, sumsq_out);
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}

extern "C" int cmb_adamw_step(const cmb_optim_job* jobs_device, int64_t n_jobs, int64_t total_chunks, float lr, float beta1,
                              float beta2, float eps, float weight_decay, float bias_correction1, float bias_correction2,
                              float grad_scale, const float* sumsq, float max_norm, void* stream) {
  const int rc = check_table(jobs_device, n_jobs, total_chunks);
  if (rc != CMB_OK) return rc;
  // (written so that a NaN fails them too)
  if (!(bias_correction1 > 0.f) || !(bias_correction2 > 0.f) || !(eps >= 0.f) || !(lr == lr) || !(grad_scale == grad_scale))
    return CMB_ERR_BAD_ARG;
  if (total_chunks == 0) return CMB_OK;
  const cmb_adamw_consts k = cmb_adamw_make(lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2);
  const float* clip = (sumsq && max_norm > 0.f) ? sumsq : nullptr;
  hipLaunchKernelGGL(adamw_step_kernel, dim3(grid_for(total_chunks)), dim3(CMB_OPTIM_THREADS), 0, (hipStream_t)stream,
                     jobs_device, n_jobs, total_chunks, k, grad_scale, clip, max_norm);
  CMB_CHECK_LAUNCH();
  return CMB_OK;
}
