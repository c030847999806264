/* tdvc.h — C ABI of libtdvc_hip.so: MI355X (gfx950) kernels for TD-VC-GAN's G+D train step.
 *
 * The reference (vicpc00/td-vc-gan) has NO native/FFI interface: its boundary is the Python
 * nn.Module surface. This ABI is what sits directly beneath that surface; each
 * entry point names the ATen operator instance(s) of the reference it replaces (file:line under
 * /root/reference). INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions (all entry points):
 *   - plain C, caller-owned DEVICE pointers, fp32, tensors [B][C][T] with T fastest; a batch stride
 *     (in elements) is passed wherever a channel-slice of a larger tensor may be used;
 *   - asynchronous on the hipStream_t passed as void* (NULL = default stream); no allocation, no
 *     synchronisation, no host read-back inside -> every call is hipGraph-capturable;
 *   - returns 0 (TDVC_OK) or a negative tdvc_status; never throws. tdvc_last_error() gives text;
 *   - re-entrant: the compute entry points keep no mutable state (per-kernel LDS-size attributes are set under
 *     std::call_once). The only process-global state is the TEST-ONLY switches tdvc_set_force_generic and
 *     tdvc_debug_*: they exist so that the parity tests can reach and name every kernel instance; the product path
 *     never calls them and they must not be flipped while another thread is launching.
 */
#ifndef TDVC_H
#define TDVC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum { TDVC_OK = 0, TDVC_EINVAL = -1, TDVC_EWORKSPACE = -2, TDVC_ELAUNCH = -3, TDVC_EUNSUPPORTED = -4 } tdvc_status;

/* Operand transform applied while a tensor is staged into LDS (fused prologue). */
typedef enum {
  TDVC_XF_NONE = 0,       /* v */
  TDVC_XF_LRELU = 1,      /* leaky_relu(v, slope)                      — nn.LeakyReLU before every G conv (model/generator.py:74,82) */
  TDVC_XF_FILM_LRELU = 2, /* leaky_relu(v*(1+gamma)+beta, slope)       — FiLM (model/generator.py:104-107) fused into posconv's load */
  TDVC_XF_MASK_LRELU = 3, /* v * (aux>0 ? 1 : slope)                   — backward of an in-place LeakyReLU (model/discriminator.py:20) */
  TDVC_XF_MASK_TANH = 4   /* v * (1-aux^2)                             — backward of nn.Tanh (model/generator.py:337,347) */
} tdvc_xform_kind;

typedef struct {
  int32_t kind;        /* tdvc_xform_kind */
  float slope;         /* LeakyReLU slope */
  float scale;         /* multiplies the transformed value (1 = none) */
  const float* aux;    /* FILM: gamma/beta tensor [B][2C][T]; MASK_*: activation output, same shape as operand */
  int64_t aux_bs;      /* batch stride of aux (elements) */
} tdvc_xform;

typedef enum { TDVC_CONV = 0, TDVC_CONV_TRANSPOSE = 1 } tdvc_conv_kind;
typedef enum { TDVC_POST_NONE = 0, TDVC_POST_LRELU = 1, TDVC_POST_TANH = 2 } tdvc_post_act;
typedef enum {
  TDVC_DG_PLAIN = 0,     /* dx = acc */
  TDVC_DG_MASK_LRELU = 1,/* dx = acc * lrelu'(x_in)                       (pre-activation conv) */
  TDVC_DG_FILM = 2       /* x_in = h: m = lrelu'(h(1+g)+b); dh2 = acc*m; dx = dh2*(1+g); dgb = [dh2*h ; dh2] */
} tdvc_dgrad_epilogue;

/* One 1-D convolution layer instance. Replaces aten::conv1d / aten::conv_transpose1d /
 * aten::convolution_backward for nn.Conv1d / nn.ConvTranspose1d / F.conv1d call sites:
 * model/generator.py:17-22,75-92,146-157,165-168,214-249,300-362 ; model/discriminator.py:17-37,100-102. */
typedef struct {
  int32_t kind;          /* tdvc_conv_kind */
  int32_t B, Cin, Cout;  /* Cin/Cout are the module's in/out channels (for transpose: x has Cin, y has Cout) */
  int32_t Tin, Tout;
  int32_t K, stride, dilation, pad, groups;
  int32_t reflect;       /* 1: padding_mode='reflect' (stride 1 only), 0: zeros */
  /* Input-channel window of the weight tensor (groups == 1, kind == TDVC_CONV): the weight is
   * [Cout][w_cin][K] and this call uses input channels [w_cin_off, w_cin_off + Cin). 0/0 = whole tensor.
   * Lets FiLM's cond_var.0 (model/generator.py:88) split into its time-constant speaker-embedding part
   * (128 channels, evaluated on a length-3 signal) and its 8-channel excitation part (SURVEY §2.2 reduction 2). */
  int32_t w_cin, w_cin_off;
} tdvc_conv_desc;

typedef struct {
  const float* x; int64_t x_bs;      /* input activation */
  tdvc_xform x_xf;                   /* prologue on x */
  const float* w;                    /* effective weight, module layout: conv [Cout][Cin/g][K]; transpose [Cin][Cout/g][K] */
  const float* bias;                 /* [Cout] or NULL */
  const float* res; int64_t res_bs;  /* optional residual added before post_act (FiLM block shortcut) */
  int32_t post_act; float post_slope;
  float out_scale;                   /* y = out_scale * post(conv+bias+res) + (add ? add : 0) */
  const float* add; int64_t add_bs;  /* optional running sum (MRF mean, model/generator.py:192-193) */
  float* y; int64_t y_bs;
  const float* bias3;                /* optional [B][Cout][3]: per-sample bias for t==0 / interior / t==Tout-1 */
  uint32_t* sign_bits; int64_t sign_bits_bs; /* optional output [B][Cout][Tout/32] (batch stride in words): bit t%32 of word t/32 =
                                        (y[b][co][t] > 0) -- a 32x smaller LeakyReLU mask source for the input-grad of the NEXT layer
                                        (tdvc_conv_dgrad_args.x_sign_bits). Needs a stride-1 conv, Tout % 32 == 0, Tout > 80, 16-byte
                                        aligned operands (TDVC_EUNSUPPORTED otherwise) */
} tdvc_conv_fwd_args;

typedef struct {
  const float* dy; int64_t dy_bs;    /* upstream gradient w.r.t. y */
  tdvc_xform dy_xf;                  /* e.g. MASK_LRELU with aux = y for post-activated layers; scale = out_scale */
  const float* w;
  const float* wt;                   /* optional: the same weight pre-transposed to [Cin(_w)][Cout][K] (stride-1, groups==1 convs);
                                        lets the input-grad kernel stream contiguous weight rows (written by tdvc_weight_norm_fwd) */
  int32_t epilogue;                  /* tdvc_dgrad_epilogue */
  const float* x_in; int64_t x_in_bs; float slope; /* tensor the forward prologue read (mask / FiLM source) */
  const float* gb; int64_t gb_bs;    /* FiLM gamma/beta (TDVC_DG_FILM) */
  float* dgb; int64_t dgb_bs;        /* FiLM gradient out [B][2C][T] (TDVC_DG_FILM) */
  const float* add; int64_t add_bs; float add_scale; /* dx += add_scale*add (residual path gradient) */
  float* dx; int64_t dx_bs;
  const uint32_t* x_sign_bits; int64_t x_sign_bits_bs; /* optional, TDVC_DG_MASK_LRELU: the sign bits of x_in as written by
                                        tdvc_conv_fwd_args.sign_bits ([B][Cin][Tin/32]); read instead of x_in (which may then be NULL).
                                        Same shape limits as sign_bits */
} tdvc_conv_dgrad_args;

typedef struct {
  const float* x; int64_t x_bs; tdvc_xform x_xf;
  const float* dy; int64_t dy_bs; tdvc_xform dy_xf;
  float* dw;        /* accumulated: dw += sum, module layout */
  float* dbias;     /* accumulated, or NULL */
  void* workspace; size_t workspace_bytes;
} tdvc_conv_wgrad_args;

int tdvc_conv_fwd(const tdvc_conv_desc* d, const tdvc_conv_fwd_args* a, void* stream);
/* Split-bf16 x6 forward (conv_fwd_x6.hip): the same result as tdvc_conv_fwd at fp32 accuracy on the bf16 matrix pipe, for 3-tap
 * stride-1 'same' convs with 65..160 input channels and Cout % 32 == 0 (FiLM cond_var.2), prologue none / LeakyReLU, bias, no
 * other epilogue operand; TDVC_EUNSUPPORTED otherwise (call tdvc_conv_fwd). The weights come pre-split into three exact bf16
 * pieces: tdvc_conv_x6_weight_planes writes tdvc_conv_x6_weight_planes_bytes() bytes from the fp32 weight [Cout][Cin][3]; redo it
 * whenever the weight changes (once per optimizer step). The image exists for Cout % 32 == 0, 1 <= Cin <= 160, K == 3 only:
 * otherwise tdvc_conv_x6_weight_planes_bytes returns 0 and tdvc_conv_x6_weight_planes TDVC_EINVAL without writing anything. */
size_t tdvc_conv_x6_weight_planes_bytes(int32_t Cout, int32_t Cin, int32_t K);
int tdvc_conv_x6_weight_planes(const float* w, int32_t Cout, int32_t Cin, int32_t K, void* planes, void* stream);
int tdvc_conv_fwd_x6(const tdvc_conv_desc* d, const tdvc_conv_fwd_args* a, const void* weight_planes, void* stream);
int tdvc_conv_dgrad(const tdvc_conv_desc* d, const tdvc_conv_dgrad_args* a, void* stream);
int tdvc_conv_wgrad(const tdvc_conv_desc* d, const tdvc_conv_wgrad_args* a, void* stream);
size_t tdvc_conv_wgrad_workspace(const tdvc_conv_desc* d);
/* Deferred weight-gradient folds. Every weight-grad entry point (tdvc_conv_wgrad, tdvc_film_cond0_bwd) ends with a fold of
 * its per-block partial slabs (in `workspace`) into dw / dbias. With tdvc_fold_defer(1) that fold is queued on the stream
 * instead of launched, and up to 24 queued folds run as ONE launch: when the queue is full, when a new fold targets a
 * gradient that is already queued, or on tdvc_fold_flush(stream). The caller then owns two duties: every call gets a
 * workspace region that stays untouched until the flush, and tdvc_fold_flush runs before anything reads dw / dbias or
 * reuses a region. Default: off (each call folds before it returns its stream position). Process-wide switch; the queues
 * are per stream. */
void tdvc_fold_defer(int on);
int tdvc_fold_flush(void* stream);
/* Drop the queued folds of `stream` WITHOUT running them: for the failure paths (a backward pass that raised, an abandoned
 * graph capture), after which the queued descriptors point into workspace regions that later calls overwrite. */
void tdvc_fold_reset(void* stream);

/* TEST-ONLY process-global switches (see the conventions above).
 * tdvc_set_force_generic: route convs to the scalar (non-MFMA) kernels, to cross-check the two code paths.
 * tdvc_debug_force_tile: pin the tile configuration of the lean stride-1 conv kernel (cfg 0..6 = <M_REP,N_REP,WM,WN> of
 *   conv_lean.hip: 0 <1,4,1,4>, 1 <2,4,1,4>, 2 <4,4,1,4>, 3 <1,1,1,4>, 4 <1,4,4,1>, 5 <3,4,1,4>, 6 <1,2,2,2>; -1 = automatic,
 *   grid-aware choice). Lets small test shapes run the instances that only large batches select.
 * tdvc_debug_force_gemm_tile: pin the tile of the generic MFMA conv kernel (conv_gemm_kernel of conv_mfma.hip: strided, grouped,
 *   transposed convs and stride-1 convs off the lean contract; forward and input-grad). cfg 0..4 = rows x columns, <M_REP,N_REP,WM,WN>:
 *   0 16x256 <1,4,1,4>, 1 32x256 <2,4,1,4>, 2 64x256 <4,4,1,4>, 3 16x64 <1,1,1,4>, 4 64x64 <1,4,4,1>; -1 = automatic choice by grid
 *   size. A pinned tile is taken whatever the row and column count of the problem: the skips of the automatic choice are grid economy, no contract of an instance.
 * tdvc_debug_trace(1) clears and starts, (2) resumes, (0) stops recording the demangled names of the conv-family kernel
 *   instantiations launched; tdvc_debug_trace_dump copies them ('\n'-separated, NUL-terminated) and returns the size needed. */
void tdvc_set_force_generic(int on);
void tdvc_debug_force_tile(int cfg);
void tdvc_debug_force_gemm_tile(int cfg);
void tdvc_debug_knob(int which, int value); /* tuning knobs for A/B measurements: 0 = XCD-aware block order of the lean conv kernel (1 = on; default 0: measured null on this path); 3 = one block per CU in the fused conditioning backward (diagnostic); 4 = 1: no sample folding of short sequences (T = 16 / 32) in the lean conv kernel; 5 = 1: exact-fp32 MFMA instead of the split-bf16 x6 weight-grad kernel (conv_wgrad_x6.hip); 6 = 1: tdvc_conv_fwd_x6 always answers TDVC_EUNSUPPORTED; 7 = 1: two instead of three resident blocks per CU in the x6 weight-grad's plan; 8 = 1 (test-only): the 16 x 64 and 32 x 64 tiles of the lean conv kernel run their one-step-ahead MFMA loop instead of the per-tap fragment ring (same bits); 9 = 1 (test-only): the lean conv kernel runs the epilogue that loads, computes and stores one float4 at a time instead of the batched one (same bits); 10 = 1 (test-only): the reflect fold of the lean conv kernel's input-grad runs every tap, and every sub-tile on the 16-row tiles, instead of the live ones only (same bits) */
void tdvc_debug_lds_cap(int bytes);   /* tuning knob: LDS bytes per block the lean kernel's chunk-size choice may use (0 = built-in) */
void tdvc_debug_trace(int on);
size_t tdvc_debug_trace_dump(char* buf, size_t cap);
/* TEST-ONLY: fill the LDS of every CU with the bit pattern `word` (e.g. 0xFFFFFFFF = a NaN) so that a kernel which reads
 * LDS it never wrote shows up as NaN in its output instead of passing on whatever finite data the last kernel left. */
int tdvc_debug_poison_lds(uint32_t word, void* stream);
/* TOOLS-ONLY: an empty dispatch (pmc_marker_kernel) that separates table entries in a rocprofv3 trace (tools/microbench_kernels.py) */
int tdvc_debug_marker(void* stream);
/* TEST-ONLY: one slab fold through the kernel every weight-grad ends with, launched at once (the deferral switch is ignored):
 *   dst[map(i)] += slab[0][i] + slab[1][i] + ... + slab[nslab-1][i]  for i < n, slab q at slab + q * stride (stride >= n).
 * Elements i < n_w go to dw, compact rows of `rowlen` mapped onto rows of `dst_row_stride` floats (equal: no mapping); elements
 * i >= n_w go to dbias[i - n_w] (n_w < 0: no bias part). Slabs are scratch: a fold of more than 8 slabs may leave partial sums
 * in them. ref = 1 runs the one-load-per-slab reference loop on its own grid instead of the production kernel; the two agree
 * bit for bit. */
int tdvc_debug_slab_fold(const float* slab, int32_t nslab, int64_t stride, int64_t n, float* dw, int32_t rowlen, int64_t dst_row_stride,
                         int64_t n_w, float* dbias, int32_t ref, void* stream);
/* TOOLS-ONLY: tdvc_debug_fold_log(1) clears and starts, (2) the same with every fold on the reference loop and its grid plan
 * (the "before" column of tools/fold_traffic.py; switch only with no fold queued), (0) stops a log with one row per fold flush outside graph capture:
 * {folds, launches, blocks, bytes moved, microseconds between two events around the launches} (the flush then waits for the
 * stream). tdvc_debug_fold_log_read copies up to cap_rows rows of 5 doubles and returns the number recorded. */
void tdvc_debug_fold_log(int on);
size_t tdvc_debug_fold_log_read(double* rows, size_t cap_rows);

/* Fused forward of one FiLM residual block (model/generator.py:96-111), narrow long-sequence case (C == 16, T % 4 == 0, T >= 512,
 * reflect padding (K-1)*dilation/2, 16-byte aligned operands; TDVC_EUNSUPPORTED otherwise -> run the two tdvc_conv_fwd calls):
 *   h = conv_kd(LeakyReLU(x)) + b1 (stored for the backward pass);  y = scale * (conv_1x1(LeakyReLU(h*(1+gamma)+beta)) + b2 + x) + add
 * gb = [gamma; beta] [B][2C][T] or NULL (no FiLM: LeakyReLU(h)); add = MRF running sum or NULL. Bit-identical to the two-launch path. */
typedef struct {
  int32_t B, C, T, K, dilation;
  const float* x; int64_t x_bs;
  const float* w1; const float* b1;        /* dilated conv [C][C][K], bias or NULL */
  float* h; int64_t h_bs;
  const float* gb; int64_t gb_bs;
  const float* w2; const float* b2;        /* 1x1 conv [C][C][1], bias or NULL */
  const float* add; int64_t add_bs;
  float scale, slope;
  float* y; int64_t y_bs;
} tdvc_film_block_args;
int tdvc_film_block_fwd(const tdvc_film_block_args* a, void* stream);

/* Fused FiLM conditioning forward (model/generator.py:86-92, 103): gb = cond_var.2(LeakyReLU(cond_var.0(c))) with
 * c = [speaker embedding (n_cond-n_var channels, constant in time) ; excitation (n_var channels)]. The time-constant part
 * enters as k3 [B][n_cond][3] (= cond_var.0 restricted to the embedding channels, evaluated on a length-3 signal, bias
 * included: left edge / interior / right edge); the excitation part is computed per tile in LDS, so the n_cond-channel
 * intermediate is written once (cv0, for the backward pass; may be NULL) and never re-read by the forward. */
typedef struct {
  int32_t B, T, n_cond, n_var, C2;      /* C2 = 2 * n_channel (gamma and beta) */
  const float* exc; int64_t exc_bs;     /* [B][n_var][T] */
  const float* w0;                      /* cond_var.0 effective weight [n_cond][n_cond][3] */
  const float* k3;                      /* [B][n_cond][3] */
  const float* w2; const float* b2;     /* cond_var.2 effective weight [C2][n_cond][3], bias [C2] */
  float* cv0; int64_t cv0_bs;           /* optional pre-activation cond_var.0 output [B][n_cond][T] */
  float* gb; int64_t gb_bs;             /* [B][C2][T] */
  float slope;
} tdvc_film_cond_args;
int tdvc_film_cond_fwd(const tdvc_film_cond_args* a, void* stream);
/* The same forward with cond_var.2 in split-bf16 x6 arithmetic (conv_fwd_x6.hip) and cond_var.0's excitation window computed per tile inside
 * that kernel: cv0 is written once (for the backward pass) and never read back, its sign bits (cv0_sign_bits [B][n_cond][T/32], optional,
 * T % 32 == 0) come out of the same registers. w2_planes = tdvc_conv_x6_weight_planes of cond_var.2's weight (a->w2 is not read).
 * Needs n_var == 8, 64 < n_cond <= 160, n_cond % 4 == 0, C2 % 32 == 0, T >= 128, T % 4 == 0; TDVC_EUNSUPPORTED otherwise. */
int tdvc_film_cond_fwd_x6(const tdvc_film_cond_args* a, const void* w2_planes, uint32_t* cv0_sign_bits, int64_t bits_bs, void* stream);

/* Backward of cond_var.0 in the split formulation, everything that consumes d_cv0 = dL/d(cond_var.0 output) in one pass:
 * dexc (input-grad wrt the excitation), the excitation window of dW (accumulated into dw0, module layout
 * [n_cond][n_cond][3]) and dk3 (adjoint of the 3-valued bias: first step, interior sum, last step). Replaces the
 * conv_wgrad + conv_dgrad + edge_sum3 calls on the same tensor. Needs T % 4 == 0, n_var == 8, n_cond <= 144. */
typedef struct {
  int32_t B, T, n_cond, n_var;
  const float* dcv; int64_t dcv_bs;     /* [B][n_cond][T] */
  const float* exc; int64_t exc_bs;     /* [B][n_var][T] */
  const float* w0;                      /* cond_var.0 effective weight [n_cond][n_cond][3] */
  float* dexc; int64_t dexc_bs;         /* [B][n_var][T], optional */
  float* dk3;                           /* [B][n_cond][3] */
  float* dw0;                           /* weight-gradient accumulator of cond_var.0, optional */
  void* workspace; size_t workspace_bytes;   /* tdvc_film_cond0_bwd_workspace() bytes: required when dw0 is given, else
                                                 optional -- with it dk3 is summed in a fixed order (same bits every run),
                                                 without it with atomics (order, and so the last bits, may vary) */
} tdvc_film_cond0_bwd_args;
size_t tdvc_film_cond0_bwd_workspace(int32_t B, int32_t T, int32_t n_cond, int32_t n_var);
int tdvc_film_cond0_bwd(const tdvc_film_cond0_bwd_args* a, void* stream);

/* Backward of the whole conditioning network behind cond_var.2's output gradient in ONE kernel (film_cond_fused_bwd.hip):
 * d_cv0 = LeakyReLU-mask * (cond_var.2 input-grad of dgb) is produced and consumed per tile on chip -- dexc, the excitation
 * window of dw0 and dk3 as in tdvc_film_cond0_bwd -- and never written to HBM. Replaces tdvc_conv_dgrad (cond_var.2) +
 * tdvc_film_cond0_bwd. The mask comes from the sign bits the forward stored (cv0_sign_bits, [B][n_cond][T/32], T % 32 == 0)
 * or, when that is NULL, from the stored fp32 cond_var.0 output (cv0). Needs T % 4 == 0, n_var == 8, n_cond <= 144,
 * C2 % 32 == 0, wt2 = cond_var.2's effective weight pre-transposed to [n_cond][C2][3]; TDVC_EUNSUPPORTED otherwise. */
typedef struct {
  int32_t B, T, n_cond, n_var, C2;
  const float* dgb; int64_t dgb_bs;                      /* [B][C2][T] */
  const float* wt2;                                      /* [n_cond][C2][3] */
  const uint32_t* cv0_sign_bits; int64_t cv0_sign_bits_bs;   /* batch stride in words; or NULL */
  const float* cv0; int64_t cv0_bs;                      /* [B][n_cond][T], read only when cv0_sign_bits is NULL */
  const float* exc; int64_t exc_bs;                      /* [B][n_var][T] */
  const float* w0;                                       /* cond_var.0 effective weight [n_cond][n_cond][3] */
  float* dexc; int64_t dexc_bs;                          /* [B][n_var][T], optional */
  float* dk3;                                            /* [B][n_cond][3] */
  float* dw0;                                            /* weight-gradient accumulator of cond_var.0, optional */
  void* workspace; size_t workspace_bytes;               /* tdvc_film_cond_bwd_workspace() bytes: required when dw0 is
                                                            given, else optional (as in tdvc_film_cond0_bwd_args) */
  float slope;
} tdvc_film_cond_bwd_args;
size_t tdvc_film_cond_bwd_workspace(int32_t B, int32_t T, int32_t n_cond, int32_t n_var);
int tdvc_film_cond_bwd(const tdvc_film_cond_bwd_args* a, void* stream);

/* k3 [B][n_cond][3] = cond_var.0 restricted to the n_const time-constant speaker-embedding channels of its input,
 * evaluated on a length-3 constant signal with the conv's zero 'same' padding (bias b0 included; w0 = effective weight
 * [n_cond][n_cond][3], emb [B][n_const]). bwd: demb [B][n_const] (optional), and the matching window of dw0 / db0 is
 * accumulated (+=, optional). Replaces three conv launches per FiLM block on a 3-sample sequence. */
int tdvc_film_k3_fwd(const float* emb, int64_t emb_bs, const float* w0, const float* b0, float* k3, int32_t B, int32_t n_const,
                     int32_t n_cond, void* stream);
int tdvc_film_k3_bwd(const float* dk3, const float* emb, int64_t emb_bs, const float* w0, float* demb, float* dw0, float* db0,
                     int32_t B, int32_t n_const, int32_t n_cond, void* stream);
/* The same for all FiLM blocks of one MRF stage (they share `emb`): nblk <= 16 weight / bias / k3 pointers as HOST arrays (read
 * before the call returns); the backward writes `demb` already summed over the blocks and accumulates each block's dw0 / db0. */
int tdvc_film_k3_multi_fwd(const float* emb, int64_t emb_bs, const float* const* w0s, const float* const* b0s, float* const* k3s,
                           int32_t nblk, int32_t B, int32_t n_const, int32_t n_cond, void* stream);
int tdvc_film_k3_multi_bwd(const float* const* dk3s, const float* emb, int64_t emb_bs, const float* const* w0s, float* demb,
                           float* const* dw0s, float* const* db0s, int32_t nblk, int32_t B, int32_t n_const, int32_t n_cond, void* stream);

/* Multi-tensor weight norm (old-style nn.utils.weight_norm, dim=0; model/generator.py:14,
 * util/__init__.py:16-20, model/discriminator.py:11): w[row] = g[row] * v[row] / ||v[row]||, one wave per
 * dim-0 slice, every weight-normed tensor of a model in ONE launch. `params` is the model's flat parameter
 * arena (v and g live in it), `w` the flat effective-weight arena; the four DEVICE tables give, per row,
 * the element offsets of v / g in `params`, of w in `w`, and the row length. */
int tdvc_weight_norm_fwd(const float* params, float* w, const int64_t* row_voff, const int64_t* row_goff,
                         const int64_t* row_woff, const int32_t* row_len, int nrows, void* stream);
/* Same, additionally writing the [Cin][Cout][K] transposed copy of selected tensors into `wt`: per row, row_tbase =
 * offset of element (ci=0, co=row, k=0) in wt, row_tstride = Cout*K, row_k = K (0 = tensor has no transposed copy). */
int tdvc_weight_norm_fwd_t(const float* params, float* w, float* wt, const int64_t* row_voff, const int64_t* row_goff,
                           const int64_t* row_woff, const int32_t* row_len, const int64_t* row_tbase,
                           const int64_t* row_tstride, const int32_t* row_k, int nrows, void* stream);
/* grads[v] (+)= g/||v|| * (dw - v <dw,v>/||v||^2), grads[g] (+)= <dw,v>/||v||; `grads` mirrors `params`. */
int tdvc_weight_norm_bwd(const float* params, const float* dw, float* grads, const int64_t* row_voff,
                         const int64_t* row_goff, const int64_t* row_woff, const int32_t* row_len, int nrows,
                         int accumulate, void* stream);

/* Fused AdamW over a flat parameter arena (torch.optim.AdamW semantics, train.py:188-189:
 * lr, betas, eps 1e-8, weight_decay 1e-2). The 1-based step count of this update comes from step_dev
 * (a DEVICE int32, so that a captured hipGraph stays valid across replays) or, if NULL, from `step`. */
int tdvc_adamw(float* p, const float* grad, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int step, const int32_t* step_dev, float grad_scale, void* stream);
/* The same with one more factor on the gradient read from DEVICE memory (clip_coef_dev[0], or NULL): the gradient-clipping
 * coefficient of tdvc_grad_clip_coef, so that clipping costs no pass over the gradients and no host synchronisation. */
int tdvc_adamw_clipped(float* p, const float* grad, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int step, const int32_t* step_dev, float grad_scale,
                       const float* clip_coef_dev, void* stream);
/* torch.nn.utils.clip_grad_norm_ on a flat gradient buffer (/root/reference/train.py:289-290, 489-490): out[0] = min(1, max_norm /
 * (grad_scale * ||grad||_2 + 1e-6)), out[1] = grad_scale * ||grad||_2 (the norm of the gradient the optimizer sees: with data
 * parallelism grad holds the all-reduced SUM and grad_scale = 1 / world). Deterministic two-pass reduction; workspace >= 1024
 * floats. The coefficient is applied by tdvc_adamw_clipped (the gradient buffer itself is left unscaled). */
int tdvc_grad_clip_coef(const float* grad, int64_t n, float max_norm, float grad_scale, float* workspace, float* out, void* stream);
/* util.roll_batches on the last axis (/root/reference/util/__init__.py:91-102, used by util.audio.add_jitter, train.py:335-336):
 * y[b][c][t] = x[b][c][(t - shift[b]) mod T], shift = int64 [B] on the device. */
int tdvc_roll_batches(const float* x, const int64_t* shift, float* y, int B, int C, int T, void* stream);
int tdvc_inc_i32(int32_t* p, int32_t by, void* stream);

/* Element-wise / reductions over [B][C][T] tensors. */
int tdvc_l2norm_fwd(const float* x, float* y, float* inv_norm, int B, int C, int T, float eps, void* stream);   /* F.normalize(dim=1), model/generator.py:271 */
int tdvc_l2norm_bwd(const float* y, const float* inv_norm, const float* dy, float* dx, int B, int C, int T, void* stream);
int tdvc_gather_ch_fwd(const float* x, const int64_t* label, float* y, int B, int C, int T, void* stream);       /* x.gather(1,label), model/discriminator.py:47-51 */
int tdvc_gather_ch_bwd(const float* dy, const int64_t* label, float* dx, int B, int C, int T, void* stream);
int tdvc_concat_cond(const float* emb, const float* exc, float* c, int B, int Ce, int Cx, int T, void* stream);   /* cat([emb.repeat(T), exc]), model/generator.py:387-399 */
int tdvc_concat_cond_bwd(const float* dc, float* demb, float* dexc, int B, int Ce, int Cx, int T, int accumulate_emb, void* stream);
/* out[b][c][0..2] = d[b][c][0], sum_{t=1..T-2} d[b][c][t], d[b][c][T-1]  (adjoint of the bias3 broadcast) */
int tdvc_edge_sum3(const float* d, float* out, int B, int C, int T, void* stream);
int tdvc_axpby(const float* a, const float* b, float* y, float alpha, float beta, int64_t n, void* stream);      /* y = alpha*a + beta*b (b may be NULL) */
int tdvc_fill(float* y, float value, int64_t n, void* stream);
int tdvc_sum_n(const float* const* srcs, int nsrc, float* y, int64_t n, void* stream);   /* y = srcs[0] + ... + srcs[nsrc-1], 1 <= nsrc <= 16 (srcs: HOST array of device pointers, read before the call returns): the gradient of a tensor with several consumers (autograd's AccumulateGrad chain) in one pass */
/* WaveNet gate of the SSL encoder's WN stack (model/ssl_encoder.py:8-15, fused_add_tanh_sigmoid_multiply):
 * acts[b][c][t] = tanh(xin[b][c][t] + g[b][c][t]) * sigmoid(xin[b][H+c][t] + g[b][H+c][t]); xin / g are [B][2H][T]
 * (g optional: NULL when the stack has no global conditioning, as in SSLEncoder), acts [B][H][T]; batch strides in elements.
 * bwd: dxin [B][2H][T] from dacts [B][H][T] (the gradient wrt g equals dxin). */
int tdvc_gate_fwd(const float* xin, int64_t xin_bs, const float* g, int64_t g_bs, float* acts, int64_t acts_bs, int B, int H, int T, void* stream);
int tdvc_gate_bwd(const float* xin, int64_t xin_bs, const float* g, int64_t g_bs, const float* dacts, int64_t dacts_bs, float* dxin,
                  int64_t dxin_bs, int B, int H, int T, void* stream);

/* InstanceNorm1d(affine=False, eps) + conditional scale/shift: y = (1+gamma)*IN(x)+beta
 * (model/conditional_instance_norm.py:4-19). gb is [B][2C][Tg] with Tg = 1 (Linear path) or T (Conv path). */
int tdvc_cin_fwd(const float* x, const float* gb, float* y, float* mean, float* rstd, int B, int C, int T, int Tg, float eps, void* stream);
int tdvc_cin_bwd(const float* x, const float* gb, const float* dy, const float* mean, const float* rstd,
                 float* dx, float* dgb, int B, int C, int T, int Tg, void* stream);

/* Loss reductions. Each writes loss_out[0] (+)= weight*loss and, where present, the gradient
 * already scaled by weight*upstream. */
int tdvc_mse_const_fwd(const float* x, int64_t n, float target, float weight, float* loss_out, void* stream);      /* F.mse_loss(x, const), train.py:273-279,329 */
int tdvc_mse_const_bwd(const float* x, int64_t n, float target, float weight, const float* upstream, float* dx, void* stream);
int tdvc_l1_fwd(const float* a, const float* b, int64_t n, float weight, float* loss_out, void* stream);          /* F.l1_loss, util/losses.py:63 */
int tdvc_l1_bwd(const float* a, const float* b, int64_t n, float weight, const float* upstream, float* da, int accumulate, void* stream);
/* All L1 terms of one loss in one launch (multiscale_feat_loss, util/losses.py:55-68: a term per discriminator feature map).
 * pairs: HOST array read before the call returns. fwd: loss_out += sum_i weight_i / n_i * sum|a_i - b_i|;
 * bwd: da_i = sign(a_i - b_i) * weight_i / n_i * upstream[0]; an entry with b == NULL zero-fills da (samples of a batched map
 * the loss does not read) and is ignored by fwd. */
typedef struct { const float* a; const float* b; float* da; int64_t n; float weight; } tdvc_l1_pair;
int tdvc_l1_multi_fwd(const tdvc_l1_pair* pairs, int npairs, float* loss_out, void* stream);
int tdvc_l1_multi_bwd(const tdvc_l1_pair* pairs, int npairs, const float* upstream, void* stream);

/* log-mel L1 (util/losses.py:28-53 + torchaudio MelSpectrogram semantics). The two GEMMs run on
 * tdvc_conv_*: STFT = Conv1d(1 -> 2F, K=n_fft, stride=hop) with the windowed DFT basis as weight over the
 * reflect-padded signal, mel projection = 1x1 Conv1d(F -> n_mels) with the filterbank as weight. These are
 * the element-wise pieces around them. spec is [B][2F][N] (real rows then imaginary rows). */
int tdvc_reflect_pad_fwd(const float* x, float* y, int B, int T, int pad, void* stream);       /* torch.stft(center=True, pad_mode='reflect') */
int tdvc_reflect_pad_bwd(const float* dy, float* dx, int B, int T, int pad, void* stream);
int tdvc_power_fwd(const float* spec, float* power, int B, int F, int N, void* stream);        /* |.|^2, power=2 */
int tdvc_power_bwd(const float* spec, const float* dpower, float* dspec, int B, int F, int N, void* stream);
int tdvc_log_l1_fwd(const float* a, const float* b, int64_t n, float floor_, float weight, float* loss_out, void* stream); /* l1(log(clamp(a)), log(clamp(b))) */
int tdvc_log_l1_bwd(const float* a, const float* b, int64_t n, float floor_, float weight, const float* upstream, float* da, void* stream);

/* Contrastive InfoNCE (util/losses.py:70-116): cosine logits, softmax, CE against class 0, both
 * directions, fused with its backward. idx_* [B][T][N] int32 are the negative positions (already skipping
 * self, util/losses.py:82-83). loss_out[0] += weight*CE; dX, dY += weight * dCE/d{X,Y} (zero them first). */
/* Softmax cross-entropy, mean over the batch (F.cross_entropy on the latent classifier's logits, train.py:302, :422).
 * fwd: *loss_out += weight * mean_b CE(logits[b], labels[b]) and the softmax probabilities go to prob [B][K];
 * bwd: dlogits = weight / B * (prob - onehot) * upstream[0]. labels are int64 class indices. */
int tdvc_cross_entropy_fwd(const float* logits, const int64_t* labels, int B, int K, float weight, float* loss_out, float* prob, void* stream);
int tdvc_cross_entropy_bwd(const float* prob, const int64_t* labels, int B, int K, float weight, const float* upstream, float* dlogits,
                           void* stream);

/* Sine + noise excitation from a frame-level F0 track (util/__init__.py:22-50, f0_to_excitation): f0 [B][n_frames] in Hz
 * (0 = unvoiced; the last frame is dropped as in the reference), output exc [B][(n_frames-1)*step]. The random draws are
 * inputs: noise_v / noise_u [B][T] standard normal (voiced / unvoiced samples), start_phase [1] in radians (device pointer). */
int tdvc_f0_to_excitation(const float* f0, const float* noise_v, const float* noise_u, const float* start_phase, float* exc,
                          int B, int n_frames, int step, float sampling_rate, int linear, void* stream);

/* YIN pitch tracker (util/yin.py:24-140, `estimate` and its `soft` variant): x [B][T] (batch stride x_bs) -> f0 [B][n_frames] in Hz,
 * 0 = non-periodic frame. Frames of L = 2*tau_max samples every `stride` samples over the signal zero-padded by L/2 on the left and
 * L/2 - 1 on the right (a signal shorter than L is zero-extended to L first); tau_min = int(sr / pitch_max), tau_max =
 * int(sr / pitch_min), stride = int(frame_stride * sr) are the caller's arithmetic. The difference function is summed directly in
 * fp32 (the reference takes it from an FFT autocorrelation). soft != 0 selects the softmax-weighted period. cmdf, when not NULL,
 * receives the cumulative-mean-normalised difference [B][n_frames][tau_max-1-tau_min]. One launch, fixed summation order.
 * TDVC_EINVAL for T < 1, stride < 1 or tau_max - 1 - tau_min < 2; TDVC_EUNSUPPORTED for tau_max > 1024. */
/* frames produced for a T-sample signal (host arithmetic only, no GPU needed); <= 0 on bad arguments */
int tdvc_yin_num_frames(int32_t T, int32_t tau_max, int32_t stride);
int tdvc_yin_f0(const float* x, int64_t x_bs, int32_t B, int32_t T, int32_t tau_min, int32_t tau_max, int32_t stride,
                float threshold, int32_t soft, float sample_rate, float* f0, float* cmdf, void* stream);

/* Backward of tdvc_yin_f0 with soft != 0: upstream gradient gy [B][n_frames] -> dx [B][T] (dense), the gradient of sum(gy * f0)
 * with respect to x. Frames that are off (no CMDF entry below the threshold), frames with f0 == 0 and frames with gy == 0
 * contribute exactly zero. The forward's intermediates are recomputed with the forward's own device code. Two launches: one block
 * per frame writes the frame gradient du [B][n_frames][2*tau_max] to the workspace, a gather sums the frames that cover each
 * sample in ascending frame order. No atomics (fixed summation order), no allocation, no synchronisation; asynchronous on
 * `stream` and graph-capturable. Every element of dx is written. Same argument checks and status codes as tdvc_yin_f0, before
 * any launch; TDVC_EWORKSPACE for a null or too small workspace (tdvc_yin_soft_bwd_workspace bytes, 0 on bad arguments). */
size_t tdvc_yin_soft_bwd_workspace(int32_t B, int32_t T, int32_t tau_max, int32_t stride);
int tdvc_yin_soft_bwd(const float* x, int64_t x_bs, int32_t B, int32_t T, int32_t tau_min, int32_t tau_max, int32_t stride,
                      float threshold, float sample_rate, const float* gy, float* dx, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Banded max-sum (Viterbi) decoder with a uniform jump floor: the temporal decoding of the reference's inference pitch tracker
 * (util/crepe.py filtered_pitch(signal, "viterbi"); torchcrepe's decode.viterbi is this programme over a +-12 bin triangular
 * transition), csrc/pitch_viterbi.hip. Generic in the lattice: the CMDF of tdvc_yin_f0 (scale < 0) or a caller's activations.
 *   x      lattice fp32 [B][F][n], rows x_bs and frames x_fs >= n elements apart, last axis dense
 *   obs[f][j] = scale * x[f][j] + prior[j]                       (prior fp32 [n], or NULL for none)
 *   band   logw fp32 [n][W], lo int32 [n], destination-major: slot k of state j is predecessor i = lo[j] + k; unused slots
 *          hold -INFINITY
 *   t(i,j) = max(logw[j][i - lo[j]], -jump) for lo[j] <= i < lo[j] + W, and -jump outside the band; jump = +INFINITY
 *          disables the floor
 *   d_0[j] = obs[0][j];  d_f[j] = obs[f][j] + max_i (d_{f-1}[i] + t(i,j)), the LOWEST i among equal maxima; the path ends
 *          in the lowest j among the maxima of d_{F-1} and is traced back; path int32 [B][F], rows path_bs apart.
 * fp32 throughout, the maximum of d_f subtracted after every frame (no argmax changes in exact arithmetic, magnitudes stay
 * bounded for any F). One launch, one block per row; no atomics, no allocation, no synchronisation: graph-capturable, and
 * bit-identical from call to call. Inputs are finite or -INFINITY; a NaN in the lattice is the caller's error.
 * The workspace holds the predecessors, uint16 [B][F][n], and for n > 144 one slice per row for a band table that does not fit
 * the LDS (sized for W = 256, since the query does not take W); the query returns 0 on arguments the decoder refuses.
 * TDVC_EINVAL for non-positive n, F or W, B < 0, W > n, jump < 0 or NaN, x_fs < n, negative strides, overlapping path rows
 * and null x, logw, lo or path; TDVC_EUNSUPPORTED for n > 1024 or W > 256; TDVC_EWORKSPACE for a null or too small workspace;
 * all of them before any launch. B == 0 is a no-op. lo lives on the device, so its entries cannot be refused without a
 * synchronisation: the kernel clamps each to [0, n - W], which keeps every band inside [0, n) (pitch.viterbi_path checks
 * a table once on the host). */
size_t tdvc_viterbi_workspace(int32_t B, int32_t F, int32_t n);
int tdvc_viterbi_path(const float* x, int64_t x_bs, int64_t x_fs, float scale, const float* prior, const float* logw,
                      const int32_t* lo, int32_t W, float jump, int32_t B, int32_t F, int32_t n, int32_t* path, int64_t path_bs,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Random parametric EQ of the data pipeline (util/contentvec/audio_corruption.py random_eq + util.eq_rms_signals, which is all that
 * data/dataset.py:68-86 corrupt_audio returns): csrc/audio_eq.hip.
 *
 * tdvc_peq_sos: the reference's params2sos in float64 on the device. gains_db, q fp32 [B][n_bands] (dB, Q factor), fc float64
 * [n_bands] in Hz, sos float64 [B][n_bands][6] in scipy's layout b0 b1 b2 a0 a1 a2 with a0 = 1. Band 0 is the low shelf, band
 * n_bands-1 the high shelf, the bands between are peaking filters (RBJ cookbook), with the reference's max(fc, 2.0) and
 * A = max(0, sqrt(g)) guards. TDVC_EINVAL for n_bands < 2. One launch, no host round trip, graph-capturable.
 *
 * tdvc_sos_filter: y[b] = the cascade sos[b] (float64 [B][n_sections][6], a0 = 1, one set per row) applied to x[b] from a zero
 * state, = scipy.signal.sosfilt(sos[b], x[b]) computed in float64 and rounded once to fp32. x, y fp32 [B][T], last axis dense,
 * rows x_bs / y_bs elements apart. match_rms != 0 multiplies each row by rms(x_row) / (rms(y_row) + 1e-8) before that rounding
 * (both sums of squares in float64, fixed order). One launch, one block per row, the serial dependence over T broken by a
 * chunked state carry; no atomics, bit-identical from call to call. 1 <= n_sections <= 16 and T >= 1, TDVC_EUNSUPPORTED
 * otherwise; B == 0 or T == 0 is a no-op. The workspace query returns 0 today (workspace may be NULL). */
int tdvc_peq_sos(const float* gains_db, const float* q, const double* fc, int32_t n_bands, double sample_rate, int32_t B,
                 double* sos, void* stream);
size_t tdvc_sos_filter_workspace(int32_t B, int32_t T, int32_t n_sections);
int tdvc_sos_filter(const float* x, int64_t x_bs, const double* sos, int32_t B, int32_t T, int32_t n_sections, int32_t match_rms,
                    float* y, int64_t y_bs, void* workspace, size_t workspace_bytes, void* stream);

/* Sample-rate conversion and segment preparation of the data pipeline (data/dataset.py:106-150 load_audio): csrc/audio_resample.hip.
 *
 * tdvc_resample: resampy's table-interpolated windowed sinc (resampy.resample with its defaults, which is what load_audio calls) as a
 * polyphase FIR. sr_new / sr_orig = L / M in lowest terms; output t reads from input n = (t*M) div L with phase (t*M) mod L:
 *     y[b][t] = sum_{j < W} bank[j*bank_tap_stride + (t mod L)*bank_col_stride] * x[b][n - left + 1 + j],
 * x[b] taken as 0 outside [0, min(n_in[b], T)). bank is float64, W taps by L columns in output order (column q holds the weights
 * of phase (q*M) mod L; resample.py builds it in numpy float64 from the interpolated filter table and stores it tap-major, strides
 * (L, 1), which makes a wave's weight loads contiguous). x fp32 [B][T], rows x_bs apart; n_in, n_out int32 [B] on the
 * device (valid input samples and outputs per row, n_out[b] <= n_out_max); y fp32, rows y_bs >= n_out_max apart. Every element of
 * y[b][0 .. n_out_max) is written, zeros at and past n_out[b]; x is never read at or past n_in[b]. Accumulated in float64 in a
 * fixed order and rounded once; no atomics, bit-identical from call to call; one launch, no synchronisation, graph-capturable.
 * The workspace (tdvc_resample_workspace bytes) receives the float64 sum of squares of the unrounded outputs of every tile of
 * tdvc_resample_tile() outputs, [B][ceil(n_out_max / tile)], which tdvc_segment takes as tile_sq. TDVC_EUNSUPPORTED for a bank
 * over 8 MiB (L * W * 8 bytes) or a ratio so small that one tile's input span does not fit the LDS; TDVC_EWORKSPACE for a null or
 * too small workspace; B == 0 or n_out_max == 0 is a no-op. */
int32_t tdvc_resample_tile(void);
size_t tdvc_resample_workspace(int32_t B, int32_t n_out_max);
int tdvc_resample(const float* x, int64_t x_bs, const int32_t* n_in, const int32_t* n_out, int32_t B, int32_t T, int32_t n_out_max,
                  const double* bank, int64_t bank_tap_stride, int64_t bank_col_stride, int32_t L, int32_t M, int32_t W,
                  int32_t left, float* y, int64_t y_bs, void* workspace, size_t workspace_bytes, void* stream);

/* tdvc_segment: the rest of load_audio in one launch. Per row b with n = min(n[b], T) samples of x[b] (fp32, rows x_bs apart):
 *     gain = 10^(normalization_db / 20) / sqrt(sum(x^2) / n)   (normalize != 0; the sum from tile_sq [B][ntiles] when given, that
 *            is from tdvc_resample's unrounded outputs, else from x[b] itself; float64, fixed order; 0 when the sum is 0)
 *     crop  [start[b], start[b] + max_segment) when n > max_segment > 0 (start clamped to [0, n - max_segment]; NULL = 0)
 *     y[b][s] = x[b][start + s] * gain * aug_gain[b] * sign(aug_sign[b]) inside the crop, 0 behind it, + noise[b][s] * noise_scale
 * computed in float64 and rounded once. aug_gain, aug_sign, noise (rows noise_bs apart) may be NULL. y is fp32 [B][S] dense and
 * written completely; gain, when not NULL, receives the float64 normalisation gain per row. max_segment <= S; with
 * max_segment == 0 (no crop) T <= S. No atomics, no synchronisation, graph-capturable. */
int tdvc_segment(const float* x, int64_t x_bs, const int32_t* n, int32_t B, int32_t T, const void* tile_sq, int32_t ntiles,
                 const int32_t* start, const float* aug_gain, const float* aug_sign, const float* noise, int64_t noise_bs,
                 double noise_scale, int32_t normalize, double normalization_db, int32_t max_segment, int32_t S, float* y,
                 double* gain, void* stream);

/* Objective evaluation (test_scripts/common/test_mcd.py): mel-cepstra of a power spectrum and exact dynamic time warping.
 *
 * tdvc_sp2mc (csrc/eval_mcep.hip): the mel-cepstrum of order `order` and warping alpha of a power spectrum P[0 .. n_fft/2]:
 *     c = irfft(log(max(P, floor)));  c[0] /= 2;  mc = freqt(c[0 .. n_fft/2], order, alpha)
 * where freqt is SPTK's frequency-transform recursion: with b = 1 - alpha^2 and g = 0 at the start, for i = -m1 .. 0 (m1 = n_fft/2)
 *     d = g;  g[0] = c[-i] + alpha d[0];  g[1] = b d[0] + alpha d[1];  g[j] = d[j-1] + alpha (d[j] - g[j-1]) for j >= 2
 * and mc = the final g[0 .. order]. This is believed to be what pysptk.sp2mc(P, order, alpha) computes; parity with an installed
 * pysptk has NOT been checked. Everything after the logarithm is linear, so the caller passes it as mat, float64
 * [order + 1][nbins] dense (evaluate.sp2mc_matrix builds it on the host by pushing unit vectors through the recursion), and the
 * device computes mc[b][f][:] = mat . log(max(P[b][f][:], floor)) with the logarithm and the sums in float64, rounded once to fp32.
 * power is addressed as power[b * p_bs + f * p_fs + k * p_ns] (elements): [B][nbins][F] of this library's STFT and a caller's
 * [F][nbins] envelope both go in without a copy. mc fp32 [B][F][order + 1] dense. One launch, one block per frame, no atomics, a
 * fixed summation order, graph-capturable. TDVC_EINVAL for negative B, F or strides, nbins < 2, order outside [0, nbins - 1], a
 * floor that is not positive and finite, null pointers; TDVC_EUNSUPPORTED for nbins > 2049 or order > 255; B == 0 or F == 0 is a
 * no-op.
 *
 * tdvc_dtw (csrc/eval_dtw.hip): exact DTW of B pairs x[b] fp32 [n[b]][D], y[b] fp32 [m[b]][D] (batch strides x_bs / y_bs, frame
 * strides x_fs / y_fs >= D, last axis dense). n, m int32 [B] on the DEVICE (NULL = N / M for every pair), clamped to [0, N] /
 * [0, M]; frames at and past n[b] / m[b] are never read. Local distance d(i, j) in fp32 from direct differences:
 *     TDVC_DTW_L2 sqrt(sum_d (x - y)^2)   (fastdtw's dist=2)      TDVC_DTW_L1 sum_d |x - y|      TDVC_DTW_SQ sum_d (x - y)^2
 *     C(0,0) = d(0,0);  C(i,j) = d(i,j) + min(C(i-1,j), C(i,j-1), C(i-1,j-1)),  the FIRST minimum in the order up, left, diagonal
 *     len(0,0) = 1;     len(i,j) = len(chosen predecessor) + 1
 * C is carried in float64. cost[b] = C(n-1, m-1) float64, length[b] = len(n-1, m-1) int32 = the number of cells of the optimal
 * path under that tie rule. path, when not NULL, int32 rows path_bs >= 2 (N + M - 1) apart: (i, j) pairs from (0, 0) to
 * (n-1, m-1), then -1 up to N + M - 1 pairs. A pair with n[b] == 0 or m[b] == 0 gets cost NaN and length 0 and nothing else is
 * written for it (its path row included). The tie order is believed to be fastdtw's; that has NOT been checked, and fastdtw is an
 * approximation (radius 1) whose cost this exact programme bounds from below. One launch, one block per pair; no atomics, no
 * allocation, no synchronisation: graph-capturable, bit-identical from call to call. The workspace holds one boundary row per pair
 * (float64 + int32 [B][M]) and, with a path, 2-bit directions [B][N][ceil(M/16)] uint32; the query returns 0 on arguments the
 * call refuses. TDVC_EINVAL for B < 0, non-positive N, M or D, an unknown metric, frame strides < D, negative strides,
 * overlapping path rows, null x, y, cost or length; TDVC_EUNSUPPORTED for N or M > 4096 or D > 64; TDVC_EWORKSPACE for a null or
 * too small workspace; all before any launch. B == 0 is a no-op.
 *
 * tdvc_fastdtw (csrc/eval_fastdtw.hip): FastDTW (S. Salvador, P. Chan, "Toward accurate dynamic time warping in linear time and
 * space", Intelligent Data Analysis 11, 2007) in the form of the `fastdtw` Python package, the call the reference's test_mcd.py
 * makes: the same algorithm, NOT the exact programme, so its cost is >= tdvc_dtw's. **Parity with an installed fastdtw package has
 * NOT been checked** (the package is not available to this repository); what the tests pin is the definition below, restated
 * literally in tests/fastdtw_ref.py. Arguments, layouts, lengths, metrics, distances (fp32 from direct differences, at every
 * level), float64 costs and the tie rule are tdvc_dtw's. For one pair x [n][D], y [m][D] and radius r >= 1:
 *   recursion   if n < r + 2 or m < r + 2: the full programme of tdvc_dtw at this level. Otherwise halve both sequences, solve the
 *               halved pair, build a window from its path and solve the programme restricted to that window.
 *   halving     x'[i] = fp32(0.5f * (x[2i] + x[2i+1])) for i < floor(n / 2); an odd last frame is dropped. The pyramid is fp32, one
 *               rounding per level; the package averages in float64. This is a stated deviation.
 *   window      every cell within Chebyshev distance r of a cell of the coarse path (cells outside the coarse grid included), each
 *               coarse cell (a, b) mapped to the fine cells (2a..2a+1, 2b..2b+1) and clipped to the fine grid; the package then
 *               scans each fine row from the previous row's first column and keeps the first contiguous run. In closed form, with
 *               n_c coarse rows and jmin(a) / jmax(a) the first / last column of the coarse path in row a, fine row i (c = i / 2)
 *               gets the columns [max(2 (jmin(max(c - r, 0)) - r), 0), min(2 (jmax(min(c + r, n_c - 1)) + r) + 1, m - 1)].
 *               The odd last fine row has c = n_c and is covered by the radius alone: hence r >= 1.
 *   programme   C(i,j) = d(i,j) + min(C(i-1,j), C(i,j-1), C(i-1,j-1)) over the cells of the window, +inf outside, C(0,0) = d(0,0),
 *               the FIRST minimum in the order up, left, diagonal (the package's tuple order); the path is traced back from
 *               (n-1, m-1) along the chosen predecessors.
 * cost[b] = C(n-1, m-1) at the finest level, length[b] = the cells of its path, path as for tdvc_dtw. A pair with n[b] == 0 or
 * m[b] == 0 gets cost NaN, length 0 and a path row of -1. One launch, one block per pair, the whole pyramid inside it; no atomics,
 * no allocation, no synchronisation: graph-capturable, bit-identical from call to call. The work is O((n + m) r) cells, a window
 * holding at most (4 r + 2) (n + m - 1). The workspace holds the fp32 pyramids, the window's row bounds and 16 bytes of directions
 * per anti-diagonal; tdvc_fastdtw_workspace is an upper bound for any lengths up to N, M (want_path does not change it) and
 * returns 0 on arguments the call refuses. TDVC_EINVAL for B < 0, non-positive N, M or D, an unknown metric, radius < 1, frame
 * strides < D, negative strides, path_bs < 2 (N + M - 1) with a path, null x, y, cost or length; TDVC_EUNSUPPORTED for N or
 * M > 16384, D > 64 or radius > 8; TDVC_EWORKSPACE for a null or too small workspace; all before any launch. B == 0 is a no-op. */
enum { TDVC_DTW_L2 = 0, TDVC_DTW_L1 = 1, TDVC_DTW_SQ = 2 };
int tdvc_sp2mc(const float* power, int64_t p_bs, int64_t p_fs, int64_t p_ns, const double* mat, int32_t B, int32_t F, int32_t nbins,
               int32_t order, float floor_, float* mc, void* stream);
size_t tdvc_dtw_workspace(int32_t B, int32_t N, int32_t M, int32_t want_path);
int tdvc_dtw(const float* x, int64_t x_bs, int64_t x_fs, const float* y, int64_t y_bs, int64_t y_fs, const int32_t* n, const int32_t* m,
             int32_t B, int32_t N, int32_t M, int32_t D, int32_t metric, double* cost, int32_t* length, int32_t* path, int64_t path_bs,
             void* workspace, size_t workspace_bytes, void* stream);
size_t tdvc_fastdtw_workspace(int32_t B, int32_t N, int32_t M, int32_t D, int32_t radius, int32_t want_path);
int tdvc_fastdtw(const float* x, int64_t x_bs, int64_t x_fs, const float* y, int64_t y_bs, int64_t y_fs, const int32_t* n, const int32_t* m,
                 int32_t B, int32_t N, int32_t M, int32_t D, int32_t metric, int32_t radius, double* cost, int32_t* length, int32_t* path,
                 int64_t path_bs, void* workspace, size_t workspace_bytes, void* stream);

/* tdvc_cheaptrick (csrc/eval_cheaptrick.hip): WORLD's CheapTrick spectral envelope (M. Morise, "CheapTrick, a spectral envelope
 * estimator for high-quality speech synthesis", Speech Communication 67, 2015; WORLD's cheaptrick.cpp / common.cpp), the
 * pyworld.cheaptrick(signal, f0, time_axis, sr, fft_size=1024) step of the reference's world_analyze, and optionally the
 * mel-cepstrum of that envelope in the same launch. **Parity with pyworld has NOT been checked** (pyworld is not available to
 * this repository); what the tests pin is the definition below. N = n_fft, h = N/2, df = fs/N; frame fr of row b is centred on
 * sample pos = fr * hop (WORLD's matlab_round(t fs + 0.001) at t = fr * 5 ms when hop = fs/200); len = the row's valid length,
 * lengths[b] clamped to [0, T] (NULL = T); lin(y, p) = y[j] + (y[j+1] - y[j]) (p - j) with j = floor(p) kept inside the array.
 *   effective F0   f = f0[b][fr] if it is finite and 3 fs/(N - 3) < f0 <= fs/4, else 500 (WORLD's kDefaultF0: an unvoiced frame).
 *                  The fs/4 cap is this library's: WORLD has none and reads out of range far above it.
 *   window         half = floor(1.5 fs/f + 0.5) (halves away from zero), k = -half .. half (2 half + 1 <= N - 3);
 *                  w[k] = 0.5 cos(pi f k/(1.5 fs)) + 0.5, w /= sqrt(sum w^2); s[k] = x[b][clamp(pos + k, 0, len - 1)] w[k]
 *                  (a row with len = 0 counts as zeros), s -= w sum(s)/sum(w); s is zero-padded to N from offset 0
 *   power          P[i] = |FFT_N(s)[i]|^2, i = 0 .. h
 *   DC correction  P[i] += lin(P, (f - i df)/df) for i < 1 + floor(f N/fs), the added values from the uncorrected P
 *   smoothing      wd = 2 f/3, bd = floor(wd N/fs) + 1, m = [P[bd] .. P[1], P[0] .. P[h], P[h-1] .. P[h-bd]], seg = cumsum(m df),
 *                  S[i] = (lin(seg, i + wd/(2 df) + bd - 0.5) - lin(seg, i - wd/(2 df) + bd - 0.5)) / wd: the mean over
 *                  [i df - wd/2, i df + wd/2] of the staircase whose steps are centred on the bins, mirrored at 0 and at Nyquist
 *   safeguard      S = max(S, floor) + 2.2e-16. WORLD instead adds 1e-12 randn to the windowed samples and 2.2e-16 |randn| to S
 *                  from its own generator; this is the deterministic counterpart, so frames of digital silence (and any bin under
 *                  the floor) differ from WORLD's
 *   lifter         C = Re FFT_N(log S extended evenly to N points); for n = 0 .. h, q = n/fs:
 *                  c[n] = C[n] sl[n] cl[n] / N, sl[0] = 1, sl[n] = sin(pi f q)/(pi f q), cl[n] = (1 - 2 q1) + 2 q1 cos(2 pi f q)
 *   envelope       env[i] = exp(Re FFT_N(c extended evenly)[i]), i = 0 .. h
 *   mel-cepstrum   irfft(log env)[n] is c[n], so tdvc_sp2mc's definition applied to env is freqt(c with c[0] halved) = G . c' with
 *                  G float64 [order + 1][h + 1] dense, the frequency transform of the unit vectors (evaluate.cheaptrick_mc_matrix):
 *                  no inverse transform, no exp and no fp32 round trip through the envelope
 * signal fp32, addressed as signal[b * s_bs + t * s_ts], samples at and past len never read; f0 fp32 at f0[b * f0_bs + fr * f0_fs];
 * env fp32 [B][F][h + 1] and mc fp32 [B][F][order + 1] dense, either may be NULL but not both, mc needs G. Float64 throughout,
 * rounded once at the store: the smoothing is a difference of running sums, so a bin 10^(r/10) under the frame's peak carries a
 * relative error of about 4e-15 * 10^(r/10) in float64 (one rounding of fp32 down to some 70 dB under the peak; in fp32 the
 * valleys of a 76 dB frame are lost outright). One launch, one block per frame, no atomics, fixed summation orders: bit-identical
 * from call to call; no allocation, no synchronisation, graph-capturable.
 * TDVC_EINVAL for negative B, F, T or strides, hop or fs < 1, a floor that is not positive and finite, a q1 that is not finite,
 * env and mc both NULL, mc without G, order outside [0, h], an fs with 500 Hz outside (3 fs/(N - 3), fs/4], null signal or f0;
 * TDVC_EUNSUPPORTED for n_fft other than 512, 1024, 2048 and for more than 2^31 - 1 frames; all before any launch.
 * B == 0 or F == 0 is a no-op. */
int tdvc_cheaptrick(const float* signal, int64_t s_bs, int64_t s_ts, const int32_t* lengths, int32_t T, const float* f0, int64_t f0_bs,
                    int64_t f0_fs, int32_t B, int32_t F, int32_t hop, int32_t fs, int32_t n_fft, double q1, double floor_,
                    const double* G, int32_t order, float* env, float* mc, void* stream);

/* tdvc_dio, tdvc_stonemask (csrc/pitch_dio.hip): WORLD's DIO F0 estimator and its StoneMask refinement (M. Morise, H. Kawahara,
 * H. Katayose, "Fast and reliable F0 estimation method based on the period extraction of vocal fold vibration of singing voice and
 * speech", AES 35th Int. Conf., 2009; WORLD's dio.cpp, stonemask.cpp, matlabfunctions.cpp), the pyworld.dio + pyworld.stonemask step
 * of the reference's world_analyze with pyworld's defaults speed = 1, channels_in_octave = 2, allowed_range = 0.1. **Parity with
 * pyworld has NOT been checked** (pyworld is not available to this repository); what the tests pin is the definition below, restated
 * literally in float64 numpy in tests/dio_ref.py. eps = 1e-12, BIG = 100000, mround(v) = (int)(v + 0.5) for v > 0 and (int)(v - 0.5)
 * otherwise (matlab_round); len = the row's valid length, lengths[b] clamped to [0, T] (NULL = T). There is no decimation (speed).
 *
 * DIO, per row:
 *   frames      F_b = len / hop + 1 (integer division), t_i = i hop / fs; frames at and past F_b are 0
 *   bands       nb = 1 + (int)(log2(f0_ceil / f0_floor) cpo), bf[k] = f0_floor 2^((k + 1)/cpo): 7 bands at 50 / 500 / 2
 *   pre-filter  y = x - mean(x[0 .. len)); c = mround(fs/50); h[i] = 0.5 - 0.5 cos(2 pi (i + 1)/(2c + 2)), i = 0 .. 2c; h = -h / sum(h),
 *               h[c] += 1; y <- sum_j h[j] y[i + c - j]: a zero-phase low-cut, zeros outside [0, len)
 *   band filter hal = mround(fs / bf[k] / 2); w = the Nuttall window of 4 hal points, 0.355768 - 0.487396 cos(2 pi u) + 0.144232 cos(4 pi u)
 *               - 0.012604 cos(6 pi u), u = j/(4 hal - 1); f[i] = sum_j w[j] y[i + 2 hal - j], i = 0 .. len - 1, zeros outside [0, len).
 *               Stated deviation (both filters): WORLD multiplies the spectra of one zero-padded FFT, a circular convolution that
 *               wraps into the first few hundred samples when the padding happens to be tight; here both are linear.
 *   events      four lists from the sequences f, -f, -(f[i+1] - f[i]) and f[i+1] - f[i] (negative- and positive-going crossings, peaks,
 *               dips): on a sequence g every i with 0 < g[i] and g[i+1] <= 0 gives fine = (i + 1) - g[i]/(g[i+1] - g[i]) (the + 1
 *               is WORLD's); consecutive fines a < b give an interval at (a + b)/2/fs of value fs/(b - a)
 *   candidate   if any list has <= 2 intervals the band has cand = 0, score = BIG/eps in every frame. Otherwise each list is
 *               interpolated linearly at t_i, extrapolated from the first segment below the first location and from the last one
 *               at and above the last location (histc + interp1: with k = the number of locations <= t_i clipped to
 *               [1, n - 1], the line through intervals k - 1 and k); cand = (((v0 + v1) + v2) + v3)/4, score = sqrt(sum (v - cand)^2/3);
 *               cand > bf[k], cand < bf[k]/2, cand > f0_ceil or cand < f0_floor give cand = 0, score = BIG; last score /= cand + eps
 *   best        per frame the candidate of the lowest score, the lowest band on a tie
 *   fix         vrm = (int)(0.5 + fs/hop/f0_floor) 2 + 1, c = (vrm - 1)/2; F_b <= vrm: every frame is 0 (WORLD leaves the array unset).
 *               step 1  base = best with the first and last vrm frames 0; s1[i] = base[i] if |(base[i] - base[i-1])/(eps + base[i])| <
 *                       allowed else 0, for i >= vrm (0 below)
 *               step 2  s2 = s1, and s2[i] = 0 where any of s1[i - c .. i + c] is 0, for c <= i < F_b - c
 *               ends    neg = every i - 1 with s2[i] == 0 != s2[i-1], pos = every i with s2[i-1] == 0 != s2[i], ascending
 *               step 3  s3 = s2; from each neg[n], j runs up to the next neg (F_b - 1 after the last), exclusive:
 *                       s3[j+1] = select(s3[j], s3[j-1], j + 1), and the run stops at the first 0
 *               step 4  s4 = s3; from each pos, last first, j runs down to the previous pos (1 before the first), exclusive:
 *                       s4[j-1] = select(s4[j], s4[j+1], j - 1), and the run stops at the first 0
 *               select(cur, past, t): ref = (3 cur - past)/2; v = the candidate of frame t nearest to ref over the bands (the lowest
 *                       band on a tie); 0 if |1 - v/ref| > allowed, else v
 *               f0 = s4, rounded once to fp32.
 * StoneMask, per frame fr with f = f0_in[b][fr] (fp32): f not finite, f <= 40 or f > fs/12 (or len == 0) gives 0. Otherwise
 *   t = fr hop / fs, half = (int)(1.5 fs/f + 1), N = 2^(2 + floor(log2(2 half + 1))); for k = -half .. half
 *   raw_k = mround((t + k/fs) fs + 0.001), sample x[clamp(raw_k - 1, 0, len - 1)], u_k = ((raw_k - 1)/fs - t)/((2 half + 1)/fs),
 *   mw = 0.42 + 0.5 cos(2 pi u) + 0.08 cos(4 pi u), dw[k] = -(mw[k+1] - mw[k-1])/2 with mw = 0 beyond both ends;
 *   M = DFT_N(x mw), D = DFT_N(x dw) from offset 0, P = |M|^2, num = Re M Im D - Im M Re D.
 *   fix(g, nh) = sum_h amp_h IF_h / (sum_h amp_h h + eps) over h = 1 .. nh with idx = mround(g N / fs h), amp = sqrt(P[idx]),
 *   IF = idx fs/N + num[idx]/P[idx] fs/2/pi (0 where P = 0); the bins are read modulo N (idx can reach N; WORLD reads out of range).
 *   tent = fix(f, 2); r = 0 if tent <= 0 or tent > 2 f, else fix(tent, min((int)(fs/2/f), 6)); |r - f| > 0.2 f gives r = f.
 *   Only the at most 8 bins named by idx are evaluated, by direct summation with the phase (idx n) mod N reduced in integers.
 *   Stated deviation: the input track is fp32, so stonemask(dio(x)) passes DIO's result through one fp32 rounding where WORLD
 *   keeps float64.
 * signal fp32 at signal[b * s_bs + t * s_ts], samples at and past len never read. tdvc_dio: f0 fp32 [B][F], rows f0_bs >= F apart,
 * F >= T / hop + 1 (every frame of a full row; columns at and past F are not touched); cand / score, each NULL or float64
 * [B][nb][F] dense: the per-band candidates and scores (0 and BIG/eps at and past F_b). tdvc_stonemask: f0_in at
 * f0_in[b * fi_bs + fr * fi_fs], f0_out fp32 rows fo_bs >= F apart; f0_out may be f0_in. Float64 arithmetic, one rounding at the
 * store; no atomics, fixed summation orders: bit-identical from call to call; no allocation, no synchronisation, graph-capturable.
 * tdvc_dio is 7 launches (tables, row mean, low-cut, the band filter twice: counting the events per 1022-sample tile, then
 * writing them behind the tiles before; candidates; one wave per row for the fix steps), tdvc_stonemask one, a block per frame.
 * The workspace holds y (8 T bytes per row), the events (512 slots per tile, kind and band: 16 nb T bytes per row, the bulk), the
 * candidates and scores; tdvc_dio_workspace returns 0 on arguments the call refuses and for B == 0. tdvc_dio_num_bands returns
 * nb, 0 when the call would refuse it.
 * TDVC_EINVAL: negative B, T, F or strides, hop or fs < 1, not 0 < f0_floor < f0_ceil finite, channels_in_octave or allowed_range not
 * positive and finite, a band at or above fs, F < T / hop + 1, overlapping output rows, null signal (with T > 0) or f0. TDVC_EUNSUPPORTED:
 * nb > 16, T > 2^21 (131 s at 16 kHz), B > 65535, a low-cut (2 mround(fs/50) + 1) or lowest-band (4 hal) filter of more than 2048 taps
 * (fs <= 51 kHz; fs / f0_floor <= 1449 at 2 channels per octave), fs/hop/f0_floor > 10^6; for tdvc_stonemask a 40 Hz window
 * (2 (int)(1.5 fs/40 + 1) + 1) of more than 4096 samples (fs <= 54 kHz), more than 2^31 - 1 frames or samples. TDVC_EWORKSPACE for a
 * null or too small workspace. All before any launch. B == 0 or F == 0 is a no-op. */
int32_t tdvc_dio_num_bands(double f0_floor, double f0_ceil, double channels_in_octave);
size_t tdvc_dio_workspace(int32_t B, int32_t T, int32_t F, int32_t hop, int32_t fs, double f0_floor, double f0_ceil,
                          double channels_in_octave);
int tdvc_dio(const float* signal, int64_t s_bs, int64_t s_ts, const int32_t* lengths, int32_t T, int32_t B, int32_t F, int32_t hop,
             int32_t fs, double f0_floor, double f0_ceil, double channels_in_octave, double allowed_range, float* f0, int64_t f0_bs,
             double* cand, double* score, void* workspace, size_t workspace_bytes, void* stream);
int tdvc_stonemask(const float* signal, int64_t s_bs, int64_t s_ts, const int32_t* lengths, int32_t T, const float* f0_in, int64_t fi_bs,
                   int64_t fi_fs, int32_t B, int32_t F, int32_t hop, int32_t fs, float* f0_out, int64_t fo_bs, void* stream);

/* Speaker similarity (csrc/eval_speaker.hip): Resemblyzer's VoiceEncoder.embed_utterance with its shipped hparams, the live path
 * of the reference's test_scripts/common/test_speaker_rec.py, restated here. Resemblyzer, librosa and webrtcvad are not available:
 * this definition is the contract and the tests pin it; PARITY WITH AN INSTALLED RESEMBLYZER / LIBROSA IS UNCHECKED.
 *   Constants: sr = 16000, n_fft = 400, hop = 160, n_mels = 40, windows of 160 frames (25600 samples), hidden size 256,
 *   embedding size 256, 3 layers.
 *   Windows (compute_partial_slices(n, rate, min_coverage), n = the row's length in samples): n_frames = ceil((n + 1) / 160),
 *   frame_step = int(round((sr / rate) / 160)) (77 at rate 1.3), steps = max(1, n_frames - 160 + frame_step + 1); window j starts at
 *   mel frame j frame_step for every j frame_step < steps and covers 160 frames, samples [160 start, 160 (start + 160)); the last
 *   window is dropped when there is more than one and (n - its first sample) / 25600 < min_coverage (float64 division). The count
 *   goes 1 -> 2 at n = 31520, 2 -> 3 at 43840, 3 -> 4 at 56160 at the defaults. The row is zero-padded to
 *   L' = max(n, last window's end). tdvc_voice_window_count is this closed form on the host, the function the kernels call.
 *   Mel front end (librosa.feature.melspectrogram(y, sr, n_fft=400, hop_length=160, n_mels=40), transposed, of the padded row):
 *   1 + L' / 160 centred frames, frame f covers padded samples [160 f - 200, 160 f + 200); reflect padding about samples 0 and
 *   L' - 1 without repeating the edge sample (pad_constant = 0; librosa < 0.10's default) or zeros (pad_constant = 1; librosa
 *   0.10 and later); samples at and past n count as zero and are never read. Periodic Hann window of 400 points, power |DFT|^2 on
 *   201 bins, NO LOGARITHM, then the 40 x 201 filterbank librosa.filters.mel(sr, 400, n_mels=40, fmin=0, fmax=sr/2, htk=False,
 *   norm='slaney'): Slaney mel scale (mel = f / (200/3) below 1000 Hz, 15 + ln(f/1000) / (ln(6.4)/27) above), 42 band edges e
 *   equally spaced in mel on 0..8000 Hz, triangles max(0, min((f_k - e_i)/(e_{i+1} - e_i), (e_{i+2} - f_k)/(e_{i+2} - e_{i+1}))) at
 *   f_k = k sr / n_fft, each row scaled by 2 / (e_{i+2} - e_i). `tables` is float64 [400 cos(2 pi i/400) | 400 sin | 400 Hann |
 *   40 x 201 filterbank], built on the host. Frames at and past 1 + L'/160 of a row are written as zeros. Float64 arithmetic,
 *   one rounding at the store.
 *   Volume (normalize_volume(wav, -30 dBFS, increase_only=True)): tdvc_voice_gain writes gain[b] = 10^((-30 - 20 log10 rms)/20)
 *   where that is > 1 and 1 otherwise, rms over the row's n samples in float64; tdvc_voice_mel multiplies the samples by it
 *   (gain = NULL: no scaling). Stated deviation: preprocess_wav's silence trimming (webrtcvad) is not reproduced.
 *   Network: torch.nn.LSTM(I, 256, layers, batch_first=True): gate order i, f, g, o; i, f, o = sigmoid, g = tanh; c' = f c + i g,
 *   h' = o tanh(c'); zero initial state; both bias vectors added. The top layer's h after the last step, then e = relu(W h + b)
 *   and e / ||e||_2 without an epsilon (an all-zero e gives NaN, as the reference). Utterance embedding: the mean over the row's
 *   kept windows of their normalised embeddings, normalised again.
 * tdvc_voice_windows: counts int32 [B] and slots int32 [B][P_max][2] = (row, start frame) from the device lengths (NULL: T);
 *   counts are clamped to P_max. tdvc_lstm_fwd: frames fp32 at frames[b f_bs + f f_fs + i], i < I <= 256; slot p is window
 *   (slots[2p], slots[2p + 1]) and covers T_steps <= 160 frames; with counts, slot p is used when p % P_max < counts[row]; a slot
 *   whose row or frames lie outside [0, B) x [0, F] is unused as well. h_out fp32 [P][256]: unused slots are ZEROED, frames no
 *   used window covers are never used (they may hold NaN). weights: 4 pointers per layer, w_ih [1024][I or 256], w_hh [1024][256],
 *   b_ih, b_hh [1024], fp32 dense. Per layer: two packing launches, the input projection of all frames as one fp32 MFMA GEMM, and
 *   the recurrence, a workgroup per 16 windows for all steps with W_hh streamed from L2; workgroups never wait for one another.
 *   tdvc_voice_embed: h [B P_max][256] -> partial [B P_max][256] (zeros for unused slots) and / or utt [B][256].
 * fp32 throughout the network, exact-fp32 MFMA, accurate expf / tanhf; no atomics, fixed summation orders: bit-identical from call
 * to call; no allocation, no synchronisation, graph-capturable.
 * TDVC_EINVAL: negative sizes or strides, frame_step or P_max < 1, NaN min_coverage, null pointers, f_fs < I. TDVC_EUNSUPPORTED:
 * I > 256, layers outside 1..3, T_steps outside 1..160, more than 2^21 frames (B F) or window steps (P T_steps), T > 2^26,
 * B > 65535 (mel, gain), reflect padding with T <= 200. TDVC_EWORKSPACE for a null or too small workspace (tdvc_lstm_workspace,
 * 0 on arguments the call refuses). All before any launch; B == 0 / P == 0 is a no-op. */
int32_t tdvc_voice_window_count(int64_t n, int32_t frame_step, double min_coverage, int64_t* padded);
int tdvc_voice_windows(const int32_t* lengths, int32_t T, int32_t B, int32_t frame_step, double min_coverage, int32_t P_max,
                       int32_t* counts, int32_t* slots, void* stream);
int tdvc_voice_gain(const float* signal, int64_t s_bs, const int32_t* lengths, int32_t T, int32_t B, double* gain, void* stream);
int tdvc_voice_mel(const float* signal, int64_t s_bs, const int32_t* lengths, int32_t T, int32_t B, int32_t F, int32_t frame_step,
                   double min_coverage, int32_t pad_constant, const double* gain, const double* tables, float* mel, void* stream);
size_t tdvc_lstm_workspace(int32_t B, int32_t F, int32_t I, int32_t P, int32_t T_steps, int32_t layers);
int tdvc_lstm_fwd(const float* frames, int64_t f_bs, int64_t f_fs, int32_t B, int32_t F, int32_t I, const int32_t* slots,
                  const int32_t* counts, int32_t P, int32_t P_max, int32_t T_steps, int32_t layers, const float* const* weights,
                  float* h_out, void* workspace, size_t workspace_bytes, void* stream);
int tdvc_voice_embed(const float* h, int32_t B, int32_t P_max, const int32_t* counts, const float* W, const float* bias,
                     float* partial, float* utt, void* stream);

/* Speaker recognition (csrc/eval_ecapa.hip): speechbrain's Fbank + sentence mean normalisation + ECAPA-TDNN embedding, the path of
 * the reference's test_scripts/mls-pt/test_speaker_rec.py (lines 58-186; the vctk script is wired the same way), restated here from
 * knowledge of speechbrain 0.5's lobes/features.py, processing/features.py, nnet/CNN.py and lobes/models/ECAPA_TDNN.py. Neither
 * speechbrain nor torchaudio is available and the reference ships no embedding_model.ckpt: this definition is the contract and
 * tests/ecapa_ref.py restates it in float64; PARITY WITH AN INSTALLED SPEECHBRAIN IS UNCHECKED, and so are the state-dict keys
 * against a real embedding_model.ckpt. Every quirk below is speechbrain's and is kept.
 *   Input: a 16 kHz waveform row of n samples; samples at and past n are never read and count as zero.
 *   Features (Fbank(n_mels=80), InputNormalization(norm_type='sentence', std_norm=False)):
 *     STFT: n_fft = win = 400, hop 160, periodic Hamming window (torch.hamming_window(400): 0.54 - 0.46 cos(2 pi i / 400)),
 *       center=True with pad_mode='constant' (zeros), one-sided 201 bins; frame count F = 1 + n / 160 (integer division).
 *     Power: re^2 + im^2 (spectral_magnitude(power=1) returns the power spectrum, not its root).
 *     Filterbank: HTK mel scale mel = 2595 log10(1 + hz/700); hz[0..n_mels+1] the image of n_mels + 2 points equally spaced in mel on
 *       0..8000 Hz; f_c[i] = hz[i+1]; band[i] = hz[i+1] - hz[i] (THE LEFT WIDTH ONLY); bin frequencies linspace(0, 8000, 201); filter
 *       i at bin frequency f is max(0, min((f - f_c[i])/band[i] + 1, -(f - f_c[i])/band[i] + 1)): a symmetric triangle of half-width
 *       band[i] with peak 1, no area normalisation.
 *     dB: 10 log10(max(x, 1e-10)), then max(., M - 80) with M the largest dB value of the row over its own F frames and all bands.
 *     Normalisation: subtract, per band, the mean over the row's F frames.
 *   Network (ECAPA_TDNN(input_size=80, channels=[C,C,C,C,3C] = [1024,1024,1024,1024,3072], kernel_sizes=[5,3,3,3,1],
 *   dilations=[1,2,3,4,1], attention_channels=128, lin_neurons=192), res2net_scale=8, se_channels=128, global_context=True, eval):
 *     Conv1d: "same"-padded with REFLECT padding, (k - 1) d / 2 per side, the edge sample not repeated, about the ROW'S OWN first and
 *       last frame (not the buffer's). TDNNBlock(x) = BatchNorm(ReLU(conv(x))), running statistics, eps 1e-5.
 *     blocks[0] = TDNNBlock(80 -> C, k5, d1). blocks[1..3] = SERes2NetBlock(C -> C, k3, d = 2, 3, 4): tdnn1 (k1); Res2Net over 8 channel
 *       chunks, y0 = x0, y1 = B0(x1), yi = B(i-1)(xi + y(i-1)), each B a TDNNBlock(C/8 -> C/8, k3, d); tdnn2 (k1); SE: s = mean over the
 *       row's frames, g = sigmoid(conv2(relu(conv1(s)))), g x; then + the block's input.
 *     MFA: x = cat(blocks[1..3] outputs) -> mfa = TDNNBlock(3C -> 3C, k1).
 *     Attentive statistics pooling over the row's frames: uniform-weight mean m and sd = sqrt(clamp(sum w (x - m)^2, 1e-12));
 *       a = conv(tanh(TDNNBlock_{9C -> A, k1}(cat[x, m, sd]))); softmax over the row's frames; weighted m, sd by the same formula -> [6C].
 *     Head: asp_bn -> fc (1x1 conv 6C -> lin_neurons) -> the embedding.
 *   Classifier(192, S): logits = normalize(e) normalize(weight)^T; the script takes softmax over S, the argmax and the target's
 *   probability, and subtracts from the k-th embedding the running mean of embeddings 1..k (mean_var_norm_emb is never put in eval
 *   mode): both are stock torch ops in td-vc-gan_amd/ecapa.py (speaker_classify, running_mean_norm).
 *   Stated deviations and limits: a row is evaluated as if alone (the reference passes one file with lengths = [1.0]); rows of fewer
 *   than 5 frames (n < 640) are refused: a reflect pad of 4 needs 5 frames (T < 640 on the host; a DEVICE length below 640 cannot be
 *   refused without a synchronisation: such a row's result is unspecified, its indices are clamped into the row); every channel count
 *   a multiple of 16 (and C of 128, so that C/8 is); inference only; the vctk script's 48 kHz resampling of a 16 kHz file is not
 *   reproduced.
 * Activations are fp32 [B][C][F] at p[b bs + c cs + f] (dense frames), so that channel slices of wider buffers work. `frames` is
 * device int32 [B] (written by tdvc_fbank) or NULL for full rows; it is clamped to [0, F]. Frames at and past a row's count are never
 * read, and never written except by tdvc_fbank, which writes them as zeros. No host synchronisation, no atomics, fixed summation
 * orders: bit-identical from call to call, a row's result does not depend on its batch; graph-capturable.
 * tdvc_fbank: signal [B] rows of T samples (row stride s_bs), lengths device int32 [B] or NULL -> feats [B][n_mels][F], F = 1 + T/160,
 *   and frames[b] = 1 + n_b/160. tables: float64 [400 cos(2 pi i/400) | 400 sin | 400 Hamming | n_mels x 201 filterbank], built on the
 *   host. Float64 inside, one rounding at the store; two passes (dB values and per-block maxima into the workspace; row maximum,
 *   floor, mean), both in fixed orders.
 * tdvc_tdnn_fwd: y = epilogue(conv(x [+ x2]) + bias [+ row_bias[b]]), w [Cout][Cin][K] with row stride w_rs (0: Cin K; larger: the
 *   first Cin K columns of wider rows), K in {1, 3, 5}, dilation 1..4; epilogue 0: none; 1: ReLU then v scale[co] + shift[co] (the
 *   folded BatchNorm: scale = gamma / sqrt(var + eps), shift = beta - mean scale); 2: that followed by tanh. x2: an optional second
 *   input added to x before the convolution; row_bias: optional [B][Cout]. y must not overlap x or x2. An implicit GEMM on
 *   v_mfma_f32_16x16x4_f32 (exact fp32): 64 output channels x 64 frames per workgroup, chunks of 32 (K = 1) or 16 input channels summed from zero
 *   and then accumulated.
 * tdvc_se_block: s = mean of x over the row's frames, g = sigmoid(w2 relu(w1 s + b1) + b2) (w1 [S][C], w2 [C][S]), out = g x +
 *   residual; gate: fp32 [B][C + S], scratch and output (the gates in the first C floats of a row, the hidden layer behind them).
 *   Four launches.
 * tdvc_asp_pool: x [B][C][F] -> pooled [B][2C] = (weighted mean | weighted sd); w_tdnn [A][3C] with bias and folded scale / shift [A],
 *   w_conv [C][A] with bias [C]. The columns C..3C of w_tdnn meet inputs that are constant over time: they become a per-row bias.
 * tdvc_ecapa_head: emb[b][e] = sum_j w[e][j] (pooled[b][j] scale[j] + shift[j]) + bias[e], w [E][N].
 * The statistics, matrix-vector products, softmax and head accumulate in float64 and round once.
 * TDVC_EINVAL: negative sizes or strides, null pointers, an epilogue outside 0..2, F != 1 + T/160, w_rs < Cin K or not a multiple of 4,
 * convolution weights that are not 16-byte aligned (the kernel loads them as float4). TDVC_EUNSUPPORTED: a channel stride above 2^27, T <
 * 640 or F < 5, a channel count (or n_mels) that is not a multiple of 16, n_mels > 128, K outside {1, 3, 5}, dilation outside 1..4,
 * C or S > 65532 (se_block), B > 65535, more than 2^20 channels or 2^24 frames, T > 2^26. TDVC_EWORKSPACE for a null or too small
 * workspace (tdvc_fbank_workspace, tdvc_asp_pool_workspace: 0 on arguments the call refuses). All before any launch; B == 0 is a
 * no-op. */
typedef struct {
  int32_t B, Cin, Cout, F, K, dilation, epilogue, reserved;
  const float* x; int64_t x_bs, x_cs;
  const float* x2; int64_t x2_bs, x2_cs;      /* NULL: no second input */
  const float* w; int64_t w_rs;
  const float* bias;                          /* [Cout] or NULL */
  const float* row_bias;                      /* [B][Cout] or NULL */
  const float* scale; const float* shift;     /* [Cout], epilogue 1 and 2 */
  float* y; int64_t y_bs, y_cs;
  const int32_t* frames;                      /* device [B] or NULL */
} tdvc_tdnn_args;
size_t tdvc_fbank_workspace(int32_t B, int32_t T, int32_t n_mels);
int tdvc_fbank(const float* signal, int64_t s_bs, const int32_t* lengths, int32_t T, int32_t B, int32_t n_mels, const double* tables,
               float* feats, int64_t f_bs, int64_t f_cs, int32_t F, int32_t* frames, void* workspace, size_t workspace_bytes, void* stream);
int tdvc_tdnn_fwd(const tdvc_tdnn_args* args, void* stream);
int tdvc_se_block(const float* x, int64_t x_bs, int64_t x_cs, const float* residual, int64_t r_bs, int64_t r_cs, int32_t B, int32_t C,
                  int32_t F, const int32_t* frames, int32_t S, const float* w1, const float* b1, const float* w2, const float* b2,
                  float* gate, float* out, int64_t o_bs, int64_t o_cs, void* stream);
size_t tdvc_asp_pool_workspace(int32_t B, int32_t C, int32_t A, int32_t F);
int tdvc_asp_pool(const float* x, int64_t x_bs, int64_t x_cs, int32_t B, int32_t C, int32_t F, const int32_t* frames, int32_t A,
                  const float* w_tdnn, const float* b_tdnn, const float* scale, const float* shift, const float* w_conv,
                  const float* b_conv, float* pooled, void* workspace, size_t workspace_bytes, void* stream);
int tdvc_ecapa_head(const float* pooled, int32_t B, int32_t N, const float* scale, const float* shift, const float* w, const float* bias,
                    int32_t E, float* emb, void* stream);

/* SSL features (csrc/ssl_wavlm.hip): the WavLM feature extractor that the reference's model/ssl_encoder.py:141-145 calls as
 * WavLM.extract_features(source)[0], from the reference's vendored wavlm/WavLM.py (W) and wavlm/modules.py (M): eval mode,
 * padding_mask=None, mask=False, the layer-norm feature extractor, layer_norm_first=True, relative position embedding with
 * gru_rel_pos=True. The reference ships the code but not the 1.2 GB checkpoint: the definition is pinned to the reference's code by a
 * fixture of its own float64 output on a small seeded configuration (tests/golden/wavlm_small.npz, tools/make_golden_wavlm.py) and
 * restated in float64 in tests/wavlm_ref.py; PARITY WITH A REAL WAVLM-LARGE.PT IS UNCHECKED (the checkpoint is absent).
 * WavLM-Large is expected to be 7 convs (512,10,5) + (512,3,2) x 4 + (512,2,2) x 2 without bias, 24 layers of width 1024 with 16
 * heads and FFN 4096, conv_pos=128, conv_pos_groups=16, num_buckets=320, max_distance=800; the checkpoint's own cfg dict rules.
 *   1. Input: a waveform row of L samples, used as it is: the reference never applies cfg.normalize (its caller would have to, and
 *      SSLEncoder does not). Rows are full length: there are NO PER-ROW LENGTHS. A row's result does not depend on its batch.
 *   2. Front end (W:378-504): per layer Conv1d without bias, LayerNorm over the channels (eps 1e-5, affine), erf-GELU; frame counts
 *      (L - k) / s + 1 per layer (integer division); a row with no frame (L < 400 for the shipped layers) is refused. Then
 *      WavLM.layer_norm over the last layer's channels, then post_extract_proj (what ret_conv=True returns).
 *   3. Positional convolution (W:514-527, 577-580): grouped Conv1d(C, C, K, padding K/2, groups G) with weight norm over dim=2:
 *      w = g v / ||v||, the norm over dims 0 and 1, one norm per tap; the last output frame is dropped (SamePad of an even K); GELU;
 *      x = x + pos.
 *   4. Layer l (W:690-715, M:504-564): h = LN(x); q = (h Wq^T + bq) d^-1/2, k = h Wk^T + bk, v = h Wv^T + bv; for head n,
 *      u = grep_linear_l(h[t, n d : (n + 1) d]) (8 values), a = sigmoid(u0 + .. + u3), b = sigmoid(u4 + .. + u7),
 *      gate = a (b grep_a_l[n] - 1) + 2; scores q_t . k_s + gate[b, n, t] bias[n][bucket(s - t)], softmax over s, times v, out_proj,
 *      + x; then x = x + fc2(gelu(fc1(LN(x)))). grep_linear and grep_a are per layer; relative_attention_bias exists in layer 0 only
 *      and every layer reuses its table.
 *   5. Bias buckets (M:417-455), evaluated on the host exactly as the reference does, in torch: n = num_buckets / 2, bucket =
 *      (rel > 0) n + (|rel| < n / 2 ? |rel| : min(n / 2 + (long)(log(float(|rel|) / (n / 2)) / log(max_distance / (n / 2)) (n - n / 2)),
 *      n - 1)); the logarithm is float32 and the cast truncates toward zero, so a float64 evaluation can differ at a bucket boundary.
 *      It becomes the device table bias_rel[H][2 T' - 1], indexed by s - t + T' - 1, cached per T'.
 *   6. Output: encoder.layer_norm after the last layer -> [B][L'][C]; output_layer = k returns layer k's output without that norm.
 * Activations are token-major fp32 [B][T][C] at p[b bs + t ts + c]. No atomics, fixed summation orders: bit-identical from call to
 * call, a row in a batch gets the bits it gets alone; no host synchronisation, graph-capturable.
 * tdvc_wavlm_gemm: y[b][t][g N + n] = epilogue((sum_k A(b, g, t)[k] w[g N + n][k] + bias[g N + n]) scale_n) [+ res[b][t][g N + n]], n < N,
 *   g < groups, w [groups N][K]; scale_n = scale for scale_lo <= g N + n < scale_hi, else 1 (the d^-1/2 of q in the fused q|k|v);
 *   epilogue 0: none, 1: erf-GELU (applied before the residual is added). A(b, g, t) is the K floats at x + b x_bs + g x_gs + t x_ts,
 *   contiguous (seg_len = 0 or K), or K / seg_len segments of seg_len floats x_ss apart. With x_ts = s Cin and K = k Cin it is a
 *   strided Conv1d over token-major input (weights permuted to [Cout][k][Cin]). res may be y itself (same strides); y must not
 *   otherwise overlap x or res. Exact fp32 on v_mfma_f32_16x16x4_f32, 64 tokens x 64 columns per workgroup, chunks of 32 summed from
 *   zero and then accumulated.
 * tdvc_wavlm_frames: the frame count after n_layers convolutions, (L - k) / s + 1 each, 0 once a row is shorter than a kernel; -1 on
 *   bad arguments. Host only.
 * tdvc_wavlm_conv0: the first convolution (one input channel; w_t [K][C], transposed), its LayerNorm and GELU: x [B] rows of L samples
 *   -> y [B][(L - K) / stride + 1][C]. Float64 inside, one rounding.
 * tdvc_wavlm_layernorm: y = LN(x) over rows of C floats (eps 1e-5, biased variance), float64 statistics, one rounding; gelu = 1
 *   applies erf-GELU. With H > 0 also gate[B][H][T] of item 4 from the normalised (stored) row, grep_w [8][C / H], grep_b [8],
 *   grep_a [H], float64 inside (a second launch). y may be x.
 * tdvc_wavlm_posconv: xp [B][T + K - 1][C] (row stride xp_bs) holds the row behind K / 2 zero tokens and in front of K / 2 - 1;
 *   w [C][K][C / groups] is the folded weight (w = g v / ||v||, evaluated in float64 and rounded once, permuted);
 *   y[b][t] = xp[b][t + K / 2] + gelu(conv + bias). One launch of the GEMM kernel in its segmented-row mode.
 * tdvc_wavlm_attention: q, k, v at p[b bs + t ts + n d + c] (q already scaled), gate [B][H][T], bias_rel [H][2 T - 1] ->
 *   out[b][t][n d + c] = sum_s softmax_s(q_t . k_s + gate[b][n][t] bias_rel[n][s - t + T - 1]) v_s. Keys in tiles of 64 with a
 *   running maximum and sum; plain fp32.
 * TDVC_EINVAL: negative sizes or strides, null pointers, strides that are not multiples of 4 floats or operands that are not 16-byte
 * aligned (gemm, posconv, attention: they move float4), a token stride below the row's width, an unknown epilogue, K not a multiple of
 * seg_len, a residual that is y with other strides. TDVC_EUNSUPPORTED: N, K, seg_len or C / groups not a multiple of 16, C not a
 * multiple of 16 or above 1024 (conv0, layernorm), a conv0 kernel above 64 taps or a row shorter than it, an odd positional kernel,
 * a head width outside {16, 32, 64}, more than 4096 tokens in the attention (82 s), B (x groups) or H > 65535, T > 2^24. All
 * before any launch; B == 0 is a no-op. */
typedef struct {
  int32_t B, T, N, K, groups, seg_len, epilogue, scale_lo, scale_hi;
  float scale;
  const float* x; int64_t x_bs, x_ts, x_ss, x_gs;
  const float* w;                             /* [groups N][K] */
  const float* bias;                          /* [groups N] or NULL */
  const float* res; int64_t r_bs, r_ts;       /* NULL: no residual */
  float* y; int64_t y_bs, y_ts;
} tdvc_wavlm_gemm_args;
int tdvc_wavlm_gemm(const tdvc_wavlm_gemm_args* args, void* stream);
int32_t tdvc_wavlm_frames(int64_t L, int32_t n_layers, const int32_t* kernels, const int32_t* strides);
int tdvc_wavlm_conv0(const float* x, int64_t x_bs, int32_t B, int32_t L, const float* w_t, int32_t K, int32_t stride, int32_t C,
                     const float* gamma, const float* beta, float* y, int64_t y_bs, int64_t y_ts, void* stream);
int tdvc_wavlm_layernorm(const float* x, int64_t x_bs, int64_t x_ts, int32_t B, int32_t T, int32_t C, const float* gamma, const float* beta,
                         int32_t gelu, float* y, int64_t y_bs, int64_t y_ts, int32_t H, const float* grep_w, const float* grep_b,
                         const float* grep_a, float* gate, void* stream);
int tdvc_wavlm_posconv(const float* xp, int64_t xp_bs, int32_t B, int32_t T, int32_t C, int32_t K, int32_t groups, const float* w,
                       const float* bias, float* y, int64_t y_bs, int64_t y_ts, void* stream);
int tdvc_wavlm_attention(const float* q, const float* k, const float* v, int64_t bs, int64_t ts, int32_t B, int32_t T, int32_t H, int32_t d,
                         const float* gate, const float* bias_rel, float* out, int64_t o_bs, int64_t o_ts, void* stream);

/* The CREPE pitch tracker (csrc/pitch_crepe.hip): what the reference's util/crepe.py filtered_pitch computes with torchcrepe's `tiny`
 * network at hop 64 (train.py:239, :549, :635; generate_with_target.py:139, :161 with "viterbi"; generate_from_list.py:101, :104),
 * restated here from torchcrepe's published source. torchcrepe is not available and no weights are shipped: this definition is the
 * contract and tests/crepe_ref.py restates it in float64 with stock torch ops. PARITY WITH AN INSTALLED TORCHCREPE AND WITH ITS
 * SHIPPED tiny.pth IS UNCHECKED, and so are the state-dict keys against a real file and `full` beyond one row. The forward; the backward
 * with respect to the signal follows below.
 *   Constants: 360 bins of 20 cents; cents(bin) = 20 bin + 1997.3794084376191; hz(cents) = 10 2^(cents / 1200);
 *     bin(hz, q) = q((1200 log2(hz / 10) - 1997.3794084376191) / 20), q = floor unless stated; sample rate 16000, window 1024.
 *   Front end (preprocess, pad=True): the row of n samples is zero-padded by 512 on both sides; F = 1 + n / hop frames (integer
 *     division) of 1024 samples every hop samples; each frame loses its mean and is divided by max(1e-10, std), std the unbiased
 *     (n - 1) standard deviation.
 *   Network (capacity tiny | full): output channels [128, 16, 16, 16, 32, 64] | [1024, 128, 128, 128, 256, 512]; six layers, each
 *     zero-pad -> conv -> ReLU -> BatchNorm in eval mode (eps 0.0010000000474974513) -> max-pool 2. Layer 1: 1 -> C1, kernel 512,
 *     stride 4, pad (254, 254): 1024 -> 256 -> 128 positions. Layers 2..6: kernel 64, stride 1, pad (31, 32): 128 -> 64 -> 32 -> 16 ->
 *     8 -> 4 positions after each pool. THE BATCHNORM COMES AFTER THE RELU AND ITS SCALE MAY BE NEGATIVE: the pool cannot be moved in
 *     front of the affine. The result [N][C6][4] is flattened POSITION-MAJOR (permute(0, 2, 1): feature l C6 + c), then
 *     Linear(4 C6, 360) and a sigmoid.
 *   Post-processing (postprocess and util/crepe.py:55-84) on activations [B][360][F]: bins below minidx = bin(fmin) and from maxidx =
 *     bin(fmax, ceil) on are excluded (39 and 248 for the reference's 50 and 550 Hz; evaluated on the host in float64).
 *     argmax: the LOWEST index among equal maxima, pitch hz(cents(bin)).
 *     weighted_argmax: around the argmax bin b the window [max(0, b - 4), min(360, b + 5)); weights sigmoid(activation) inside the
 *       window and in range, 0 elsewhere (torchcrepe's second sigmoid on values that are already probabilities, kept); pitch
 *       hz(sum w cents / sum w).
 *     viterbi: observation = log-softmax over the in-range bins; transition max(12 - |i - j|, 0) row-normalised over all 360 bins;
 *       uniform initial distribution; decoded by tdvc_viterbi_path on the maxidx - minidx in-range states with jump = +INFINITY; pitch
 *       hz(cents(bin)) of the path. This equals librosa's programme whenever that avoids its `tiny`-floored transitions, which it
 *       always does: staying on a state is always possible at finite cost.
 *     periodicity = the activation at the chosen bin; pitch = 0 where periodicity < threshold (0.21).
 *     get_shift(src, tgt) = bin(tgt) - bin(src).
 *   STATED DEVIATION: torchcrepe adds a random triangular dither of +-20 cents to every bin -> cents conversion; here the conversion is
 *     deterministic (the dither's mean).
 *   Decisions where the source leaves room: a row with per-row lengths is framed as if it were alone (samples at and past its length
 *     count as zero and are never read); its frames past 1 + length / hop are zero frames, their activations are those of a zero frame,
 *     and the decoders give pitch 0 and periodicity 0 there. The comparison with the threshold is made in fp32.
 * tdvc_crepe_frames: signal [B] rows of T samples (row stride s_bs), lengths device int32 [B] or NULL -> frames fp32 [B][F][1024], F = 1 +
 *   T / hop. Mean and standard deviation in float64 (two passes; per-wave butterflies, the four waves combined pairwise), one rounding
 *   at the store. A constant frame gives exactly 0.
 * tdvc_crepe_conv: one layer, x [N][Cin][Lin] -> y [N][Cout][Lc / 2] dense, Lc = 256 for (Cin 1, K 512, stride 4, Lin 1024), Lc = Lin
 *   for (K 64, stride 1, Lin in {128, 64, 32, 16, 8}); w [Cout][Cin][K]; y = maxpool2(relu(conv(x) + bias) scale + shift), scale =
 *   gamma / sqrt(var + eps), shift = beta - mean scale (evaluated in float64 on the host and rounded once). An implicit GEMM on
 *   v_mfma_f32_16x16x4_f32 (exact fp32): 16 output channels x 256 (frame, position) columns per workgroup, chunks of 128 products
 *   summed from zero and then accumulated. y must not overlap x.
 * tdvc_crepe_head: x [N][C][P] -> act[n / F][o][n % F] = sigmoid(sum_{l, c} w[o][l C + c] x[n][c][l] + bias[o]), w [O][P C]; N a
 *   multiple of F (F = 1: act [N][O]). Float64 sums in a fixed order, one rounding.
 * tdvc_crepe_decode: act at p[b a_bs + k a_cs + f]; the in-range bins are [lo, hi). mode TDVC_CREPE_ARGMAX / TDVC_CREPE_WEIGHTED write
 *   pitch and periodicity fp32 [B][F]; `bins` (device int32 [B][F] or NULL, mode ARGMAX only; clamped into [lo, hi)) replaces the
 *   kernel's own argmax (the Viterbi path); `frames` (device int32 [B] or NULL, clamped to [0, F]): frames at and past it give 0, 0.
 *   mode TDVC_CREPE_LATTICE writes lattice fp32 [B][F][hi - lo] = act - logsumexp over [lo, hi) (float64 inside, one rounding) and
 *   ignores frames, bins, pitch and periodicity. Cents -> Hz in float64, rounded once.
 * Every entry takes a stream; no atomics, fixed summation orders: bit-identical from call to call; no allocation, no host
 * synchronisation, graph-capturable. TDVC_EINVAL: negative sizes or strides, null pointers, F != 1 + T / hop, N not a multiple of F, an
 * unknown mode, bins with another mode than ARGMAX, a bin stride below F, conv weights that are not 16-byte aligned.
 * TDVC_EUNSUPPORTED: hop < 1, a row with no sample (T < 1), B > 65535, T > 2^28, a conv geometry other than the two above, Cout or (K
 * 64) Cin not a multiple of 16, head C not a multiple of 16 or O of 4, more than 2^16 output channels, 2^22 frames or 2^31 elements
 * of one operand, an empty bin range or one that leaves [0, n_bins), more than 4096 bins, F > 2^24. All before any launch; B == 0 /
 * N == 0 is a no-op. */
enum { TDVC_CREPE_ARGMAX = 0, TDVC_CREPE_WEIGHTED = 1, TDVC_CREPE_LATTICE = 2 };
typedef struct {
  int32_t N, Cin, Cout, Lin, K, stride, reserved0, reserved1;
  const float* x;                             /* [N][Cin][Lin] */
  const float* w;                             /* [Cout][Cin][K] */
  const float* bias; const float* scale; const float* shift;      /* [Cout] */
  float* y;                                   /* [N][Cout][Lc / 2] */
} tdvc_crepe_conv_args;
int tdvc_crepe_frames(const float* signal, int64_t s_bs, const int32_t* lengths, int32_t T, int32_t B, int32_t hop, int32_t F,
                      float* frames, void* stream);
int tdvc_crepe_conv(const tdvc_crepe_conv_args* args, void* stream);
int tdvc_crepe_head(const float* x, int32_t N, int32_t C, int32_t P, const float* w, const float* bias, int32_t O, int32_t F,
                    float* act, void* stream);
int tdvc_crepe_decode(const float* act, int64_t a_bs, int64_t a_cs, int32_t B, int32_t F, int32_t n_bins, int32_t lo, int32_t hi,
                      int32_t mode, float threshold, const int32_t* frames, const int32_t* bins, float* pitch, float* periodicity,
                      float* lattice, void* stream);

/* The backward of the CREPE tracker with respect to the signal (csrc/pitch_crepe_bwd.hip; tdvc_crepe_conv_train in pitch_crepe.hip): the
 * reference's activation-MSE F0 term, train.py:439-470, g_loss_f0 = mse(activations(fake), target activations). The network is fixed:
 * no weight gradient. Nothing of the forward is kept but the pooling decisions and the final activations.
 * tdvc_crepe_conv_train: tdvc_crepe_conv (the same kernel template, y bit-identical) that also writes code uint8 [N][Cout][Lc / 2]. With
 *   z = conv + bias and v = relu(z) scale + shift at the position pair (2m, 2m + 1): the odd position wins only if v_odd > v_even (on a
 *   tie the even one, as torch.max_pool2d's backward); code = 0 if the winner's z <= 0, else 1 (even winner) or 2 (odd winner).
 * tdvc_crepe_conv_bwd: dy [N][Cout][Lc / 2], code, scale [Cout] -> dx [N][Cin][Lin] in one launch: dz[n][co][p] = dy[n][co][p >> 1]
 *   scale[co] where code[n][co][p >> 1] == 1 + (p & 1), else 0 (a select: an unselected dy may hold anything); K 64, stride 1:
 *   dx[n][ci][s] = sum_co sum_k w[co][ci][k] dz[n][co][s + 31 - k]; K 512, stride 4: dx[n][s] = sum_co sum_p w[co][s + 254 - 4 p]
 *   dz[n][co][p] over 0 <= s + 254 - 4 p < 512; terms outside [0, Lc) are zero. An implicit GEMM on v_mfma_f32_16x16x4_f32, chunks
 *   summed from zero and then accumulated. wt is the packed weight: K 64: wt[ci][co][k'] = w[co][ci][63 - k'] ([Cin][Cout 64]); K 512:
 *   wt[r][co][i] = w[co][r + 510 - 4 i] where that tap exists, else 0 ([16][Cout 136]). wt and dx 16-byte aligned.
 * tdvc_crepe_head_bwd: act [B][O][F] (N = B F frames, frame n = b F + f), w [O][P C] -> dx [N][C][P], dx[n][c][l] = sum_o dlogit[n][o]
 *   w[o][l C + c] in float64, rounded once. Loss form (target and gL given, dact NULL): dlogit = gL[0] 2 (act - target) / (N O) act
 *   (1 - act), target[b][o][f] at target[b t_bs + o t_cs + f t_fs], gL a DEVICE pointer to the upstream gradient. Plain form (dact dense
 *   [B][O][F] given, target and gL NULL): dlogit = dact act (1 - act).
 * tdvc_crepe_act_mse: out[0] = mean((act - target)^2) over [B][O][F], float64, a fixed order without atomics (written, not added).
 * tdvc_crepe_frames_bwd: g [B][F][1024] (the gradient of the normalised frames) -> dsignal [B] rows of T (row stride d_bs). For a frame
 *   with y = (x - mean) / den, den = max(1e-10, std): dxf = (g - mean(g) - y sum(g y) / 1023) / den if std > 1e-10, else (g - mean(g)) /
 *   den; dsignal[b][q] = sum_f dxf[b][f][q - f hop + 512] over the frames that cover q, a gather in frame order, float64, one rounding.
 *   Samples of the zero padding receive nothing. Rows are full length (no per-row lengths). Two launches; the workspace holds four
 *   float64 per frame.
 * tdvc_roll_bins: y[b][k][f] = x[b][(k - shift[b]) mod C][f] (util.roll_batches(x, shift, 1)); x at x[b x_bs + k x_cs + f], y dense, shift
 *   device int64 [B].
 * Every entry takes a stream; no atomics, fixed summation orders, no host synchronisation, graph-capturable. Refusals as the forward's
 * (TDVC_EINVAL null pointers, negative sizes; TDVC_EUNSUPPORTED geometry other than the six layers', channel counts not multiples of
 * 16, 2^31 elements of one operand or more, more than 512 head outputs; TDVC_EWORKSPACE), all before any launch. */
typedef struct {
  int32_t N, Cin, Cout, Lin, K, stride, reserved0, reserved1;
  const float* dy;                            /* [N][Cout][Lc / 2] */
  const uint8_t* code;                        /* [N][Cout][Lc / 2] */
  const float* scale;                         /* [Cout] */
  const float* wt;                            /* the packed weights, above */
  float* dx;                                  /* [N][Cin][Lin] */
} tdvc_crepe_conv_bwd_args;
int tdvc_crepe_conv_train(const tdvc_crepe_conv_args* args, uint8_t* code, void* stream);
int tdvc_crepe_conv_bwd(const tdvc_crepe_conv_bwd_args* args, void* stream);
int tdvc_crepe_head_bwd(const float* act, const float* target, int64_t t_bs, int64_t t_cs, int64_t t_fs, const float* gL, const float* dact,
                        const float* w, int32_t N, int32_t C, int32_t P, int32_t O, int32_t F, float* dx, void* stream);
size_t tdvc_crepe_act_mse_workspace(void);
int tdvc_crepe_act_mse(const float* act, const float* target, int64_t t_bs, int64_t t_cs, int64_t t_fs, int32_t B, int32_t O, int32_t F,
                       float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t tdvc_crepe_frames_bwd_workspace(int32_t B, int32_t F);
int tdvc_crepe_frames_bwd(const float* signal, int64_t s_bs, int32_t T, int32_t B, int32_t hop, int32_t F, const float* g, float* dsignal,
                          int64_t d_bs, void* workspace, size_t workspace_bytes, void* stream);
int tdvc_roll_bins(const float* x, int64_t x_bs, int64_t x_cs, const int64_t* shift, float* y, int32_t B, int32_t C, int32_t F, void* stream);

/* The Whisper ASR metric (csrc/asr_whisper.hip): the transcripts that the reference's test_scripts/common/test_asr.py takes from
 * WhisperForConditionalGeneration("openai/whisper-medium").generate with a forced language and task, greedy, before WER and CER.
 * The definition is HF transformers' WhisperForConditionalGeneration in eval mode plus WhisperFeatureExtractor's numpy path, restated
 * here; it is pinned to that implementation's own float64 output on a small seeded configuration (tests/golden/whisper_small.npz,
 * tools/make_golden_whisper.py) and restated in float64 in tests/whisper_ref.py. No checkpoint is available and none is shipped:
 * PARITY WITH A REAL WHISPER-MEDIUM CHECKPOINT IS UNCHECKED. d_model is a multiple of 16 up to 1024 (whisper-large, d = 1280, is
 * refused), head widths 16, 32, 64. The tokenizer and Whisper's text normaliser are not reproduced: ids in, ids out.
 *   1. Features: a 16 kHz row, zero-padded or truncated to n_samples = chunk_length 16000; per-row device lengths mark where the
 *      zeros start. Periodic Hann window of 400, hop 160, center=True with reflect padding of 200, the last frame dropped:
 *      n_samples / 160 frames. Power spectrum over 201 bins, the Slaney-scale, Slaney-normalised mel filter bank (80 bands, 0 to
 *      8000 Hz; the table is built on the host in float64), log10(max(., 1e-10)), max(., rowmax - 8) with rowmax over the whole row's
 *      [n_mels][frames], (. + 4) / 4. Float64 inside, one rounding at the store. (HF's numpy path stores the spectrum as complex64
 *      before the power and rounds the log10 values to float32 before the clamp, which it then evaluates in float32; the definition
 *      does neither, and differs from HF's values by those roundings: below 2.5e-7 per value.)
 *   2. Encoder: gelu(conv1) (k 3, pad 1, n_mels -> d), gelu(conv2) (k 3, stride 2, pad 1) + embed_positions.weight (from the state
 *      dict), then encoder_layers pre-norm layers x += out_proj(attn(LN(x))) with q = (h Wq^T + bq) d_h^-1/2, k = h Wk^T WITHOUT bias,
 *      v = h Wv^T + bv and a plain softmax, x += fc2(gelu(fc1(LN(x)))); a final layer_norm. LayerNorm eps 1e-5, erf-GELU.
 *      T_enc = frames / 2. The convolutions, projections and norms are tdvc_wavlm_gemm and tdvc_wavlm_layernorm.
 *   3. Decoder step at position p for token t: x = embed_tokens[t] + embed_positions[p] (scale_embedding false); per layer causal
 *      self-attention over the cache positions 0 .. p (this step's k and v appended), cross-attention over the T_enc encoder keys and
 *      values (projected once per utterance with encoder_attn.k_proj / v_proj), the MLP; the final layer_norm and
 *      logits = x embed_tokens^T (the tied proj_out, no bias).
 *   4. Greedy generation: prompt_ids [P] go through the same step with the pick forced; then the argmax with the lowest index on
 *      ties, after -inf on the `suppress` tokens at every step and on the `begin_suppress` tokens at the first generated step (both as
 *      one byte mask [vocab]: bit 0 always, bit 1 at the first generated step); a row that has emitted eos emits pad from then on.
 *      ids [B][P + max_new_tokens], n_tokens [B] (prompt and eos included). No beams, temperature fallback, timestamps or long-form
 *      chunking; audio past chunk_length is truncated.
 *   5. WER / CER are host functions on strings (td-vc-gan_amd/whisper.py); text never lives on the device.
 * The step launches take B <= 16 rows and read the position p from a DEVICE counter: one step is the same launch sequence for every
 * p, a linear chain, without host synchronisation, and can be captured into a graph once and replayed. No atomics, fixed summation
 * orders: bit-identical from call to call, and a row in a batch gets the bits it gets alone.
 * tdvc_whisper_log_mel: item 1. x [B] rows of L samples (x_bs apart), lengths [B] or NULL (samples at and past min(lengths[b], L,
 *   n_samples) are never read), table = float64 cos[400] | sin[400] | window[400] | filterbank[n_mels][201] ->
 *   y[b y_bs + m y_ms + f y_fs] fp32, m < n_mels, f < n_samples / 160. Two launches (the row maximum needs the first to end);
 *   workspace from tdvc_whisper_log_mel_workspace.
 * tdvc_whisper_attention: q, k, v at p[b bs + t ts + n d + c] (q already scaled) -> out[b][t][n d + c] = sum_s softmax_s(q_t . k_s) v_s:
 *   the tile of tdvc_wavlm_attention without gate and bias table, T <= 4096.
 * tdvc_whisper_embed: x[b][:] = embed_tokens[ids[b][p]] + embed_positions[p], p = *pos (clamped to max_pos - 1, ids to the vocabulary).
 * tdvc_whisper_linear_step: y[b][n] = epilogue((LN?(x[b]) . w[n] + bias[n]) scale_n) [+ res[b][n]], b < B <= 16, w [N][K], exact fp32 on
 *   v_mfma_f32_16x16x4_f32 with the batch as the MFMA's 16 rows. The weights go from global memory straight to registers (each is
 *   used once); only the input rows sit in LDS; K is split over the 8 waves of a workgroup in pieces of 128 and the waves' sums are
 *   added in the order 0 .. 7. gamma, beta: the LayerNorm prologue over the row (K <= 1024, float64 statistics, one rounding,
 *   recomputed per workgroup). epilogue 0: none, 1: erf-GELU (before the residual). With k_cache the columns n >= cache_lo are k | v of
 *   width (N - cache_lo) / 2 each and go to cache[b c_bs + p (N - cache_lo) / 2 + c], p = *pos, instead of y. y must not be x; res
 *   may be y. There is no split of K across workgroups: a launch with N = d has d / 16 workgroups.
 * tdvc_whisper_attn_step: out[b][n d + c] = sum_s softmax_s(q[b][n d :] . k[b][s][n d :]) v[b][s][n d + c] over s < len' keys,
 *   len' = min(*pos + 1, len) with pos, else len; k, v at p[b kv_bs + s kv_ts + n d + c]. Keys at and past len' are never read.
 *   A workgroup per (row, head); the keys are split over 8 waves whose running maxima and sums are combined in the order 0 .. 7.
 * tdvc_whisper_logits: LN(x) embed_tokens^T through the same kernel, any vocab (the last column tile may be partial). logits (may be
 *   NULL) receives the raw values; the partials receive, per workgroup and row, the (max, lowest argmax) after the mask of item 4
 *   (mask may be NULL), the first generated step being *pos == n_prompt - 1.
 * tdvc_whisper_pick: reduces the partials in a fixed order with lowest-index ties and, with p = *pos: p + 1 < n_prompt keeps the
 *   prompt token ids[b][p + 1]; else ids[b][p + 1] = finished[b] ? pad : argmax, and an eos sets finished[b]; n_tokens[b] = p + 2
 *   for a row that was not finished; all_done[0] = every row finished; *pos = p + 1. Nothing happens once p + 1 >= total.
 * tdvc_whisper_workspace: the bytes of the self-attention cache (2 layers B max_len d floats), the cross keys and values
 *   (2 layers B T_enc d floats) and the partials; offsets[0..2] receive where each starts, offsets[3] the partials per row.
 * TDVC_EINVAL: negative sizes or strides, null pointers where not allowed, strides that are not multiples of 4 floats, operands that
 * are not 16-byte aligned, a row stride below the row's width, a cache row shorter than its positions, a short workspace, y == x.
 * TDVC_EUNSUPPORTED: d, N or K not a multiple of 16, d (or a LayerNorm row) above 1024, a head width outside {16, 32, 64}, B > 16 in a
 * step launch, more than 4096 keys, n_samples not a multiple of 160 or below 400, more than 128 mel bands. All before any launch;
 * B == 0 is a no-op. Whether p stays inside the cache is the host's to know (P + max_new_tokens <= max_target_positions is checked
 * in whisper.py); the kernels clamp p instead of writing out of bounds. */
typedef struct {
  int32_t B, N, K, epilogue, scale_lo, scale_hi;
  float scale;
  const float* x; int64_t x_bs;
  const float* gamma; const float* beta;      /* both or neither */
  const float* w;                             /* [N][K] */
  const float* bias;                          /* [N] or NULL */
  const float* res; int64_t r_bs;             /* NULL: no residual */
  float* y; int64_t y_bs;
  int32_t cache_lo, cache_len;                /* with k_cache: first cached column, positions per cache row */
  const int32_t* pos;
  float* k_cache; float* v_cache; int64_t c_bs;
} tdvc_whisper_linear_args;
size_t tdvc_whisper_log_mel_workspace(int32_t B, int32_t n_samples, int32_t n_mels);
int tdvc_whisper_log_mel(const float* x, int64_t x_bs, const int32_t* lengths, int32_t B, int32_t L, int32_t n_samples, const double* table,
                         int32_t n_mels, float* y, int64_t y_bs, int64_t y_ms, int64_t y_fs, void* workspace, size_t workspace_bytes,
                         void* stream);
int tdvc_whisper_attention(const float* q, const float* k, const float* v, int64_t bs, int64_t ts, int32_t B, int32_t T, int32_t H, int32_t d,
                           float* out, int64_t o_bs, int64_t o_ts, void* stream);
int tdvc_whisper_embed(const int32_t* ids, int64_t ids_ld, const int32_t* pos, int32_t max_pos, const float* embed_tokens,
                       const float* embed_positions, int32_t B, int32_t d, int32_t vocab, float* x, int64_t x_bs, void* stream);
int tdvc_whisper_linear_step(const tdvc_whisper_linear_args* args, void* stream);
int tdvc_whisper_attn_step(const float* q, int64_t q_bs, const float* k, const float* v, int64_t kv_bs, int64_t kv_ts, const int32_t* pos,
                           int32_t len, int32_t B, int32_t H, int32_t d, float* out, int64_t o_bs, void* stream);
size_t tdvc_whisper_workspace(int32_t d, int32_t decoder_layers, int32_t vocab, int32_t B, int32_t T_enc, int32_t max_len, int64_t* offsets);
int tdvc_whisper_logits(const float* x, int64_t x_bs, const float* gamma, const float* beta, const float* embed_tokens, int32_t B, int32_t d,
                        int32_t vocab, const uint8_t* mask, const int32_t* pos, int32_t n_prompt, float* logits, int64_t l_bs, void* partials,
                        size_t partial_bytes, void* stream);
int tdvc_whisper_pick(const void* partials, size_t partial_bytes, int32_t vocab, int32_t B, int32_t* ids, int64_t ids_ld, int32_t n_prompt,
                      int32_t total, int32_t eos, int32_t pad, int32_t* pos, int32_t* n_tokens, int32_t* finished, int32_t* all_done, void* stream);

int tdvc_contrastive_fwd_bwd(const float* X,const float* Y, const int32_t* idx_x, const int32_t* idx_y, int B, int C, int T, int N,
                             float weight, float* loss_out, float* dX, float* dY, void* stream);

const char* tdvc_last_error(void);
int tdvc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TDVC_H */
