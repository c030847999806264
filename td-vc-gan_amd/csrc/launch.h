// Host functions that one translation unit defines and another calls, declared once. Every defining .hip includes this
// header too, so a definition that drifts from its declaration does not compile.
#pragma once
#include "conv_common.h"
#include "conv_wgrad_lean.h"

namespace tdvc {

// conv_mfma.hip: generic conv kernels (MFMA window-GEMM, scalar), their weight-grads and the slab folds
template <int MODE> hipError_t launch_conv_gemm(GemmConvP p, int B, hipStream_t st);
template <int MODE> hipError_t launch_conv_scalar(GemmConvP p, int B, hipStream_t st);
template <int MODE> hipError_t launch_conv_wgrad(WgradP p, int B, int bpb, hipStream_t st);
template <int MODE> hipError_t launch_conv_wgrad_scalar(WgradP p, int B, long nweights, float* dw, hipStream_t st);
int wgrad_geometry(WgradP& p, int B, int* bpb_out);
bool wgrad_mfma_supported(int J);
hipError_t launch_slab_reduce(const float* slab, int nslab, long stride, long n, float* dw, int rowlen, long dst_row_stride,
                              hipStream_t st, long n_w = -1, float* dbias = nullptr);
hipError_t launch_bias_grad(const Opnd& a, int N, int Ctot, int B, float* dbias, hipStream_t st);
hipError_t fold_flush(hipStream_t st);
void fold_set_defer(int on);
void fold_reset(hipStream_t st);
hipError_t debug_slab_fold(const float* slab, int nslab, long stride, long n, float* dw, int rowlen, long dst_row_stride, long n_w,
                           float* dbias, int ref, hipStream_t st);
void fold_log_set(int on);
size_t fold_log_read(double* rows, size_t cap_rows);

// conv_wgrad_lean.hip
void wgrad_lean_plan(int R, int Cin, int N, int K, int B, int* ntiles, int* tpb, int* ngroups);
int wgrad_lean_nslab(int R, int Cin, int N, int K, int B);

// conv_wgrad_x6.hip
bool wgrad_x6_ok(int R, int Cin, int T, int K, int dil, int pad, int reflect);
void wgrad_x6_plan(int R, int T, int B, int* ntiles, int* tpb, int* ngroups);
hipError_t launch_conv_wgrad_x6(const WgLeanP& q, int B, hipStream_t st);

// film_cond_bwd.hip: host side shared by tdvc_film_cond0_bwd and tdvc_film_cond_bwd. Both kernels walk `tpb` consecutive
// (sample, chunk) pairs per block, leave one 24 x n_cond dW slab per block and one 3 x n_cond dk3 slot per (block, sample).
hipError_t launch_dk3_fold(const float* slots, float* dk3, int B, int nc, int ntile, int tpb, hipStream_t st);
struct FilmCondPlan { int ntile, tpb, nblocks; size_t slab_floats, slot_floats; };
FilmCondPlan film_cond_plan(int B, int T, int n_cond, int chunk);
struct FilmCondBwdHost {
  const char* who;                     // entry point name, prefix of its error messages
  int B, T, n_cond, n_var; float* dk3; float* dw0; void* workspace; size_t workspace_bytes; hipStream_t st;
  FilmCondPlan pl;                     // begin() fills these: the kernel's grid plan and workspace pointers
  float* slab; long slab_stride; float* dk3_slots;
  int begin(int chunk);                // workspace check and split, dk3 zeroed when it has no slots
  int finish();                        // after the kernel: dk3 fold, slab fold into the excitation window of dw0
};

}  // namespace tdvc
