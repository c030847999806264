// C-ABI entry points for the convolution family: maps a (tdvc_conv_desc, args) pair onto the
// reduced stride-1 problem of conv_common.h and picks the MFMA or the scalar kernel.
#include "../../include/tdvc.h"
#include "launch.h"
#include "conv_lean.h"
#include "conv_small_group.h"
#include "api_util.h"

using namespace tdvc;

static inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static inline bool ok_bs(const void* p, long bs) { return !p || (bs < (1L << 31)); }
static inline bool vec_ptr(const void* p, long bs) { return !p || (al16(p) && (bs & 3) == 0); }
static inline float scale_or_1(float s) { return s == 0.f ? 1.f : s; }   // ABI: a scale of 0 means unset

// Prologue kind of the lean kernel for an operand transform; -1 = not supported there.
static int lean_xfk(const tdvc_xform& x, float* slope, float* scale, const float** aux, long* aux_bs) {
  *scale = scale_or_1(x.scale); *aux = x.aux; *aux_bs = x.aux_bs; *slope = x.slope;
  switch (x.kind) {
    case TDVC_XF_NONE: *slope = 1.f; *aux = nullptr; return LXF_ACT;
    case TDVC_XF_LRELU: *aux = nullptr; return (x.slope >= 0.f && x.slope <= 1.f) ? LXF_ACT : -1;
    case TDVC_XF_FILM_LRELU: return (x.slope >= 0.f && x.slope <= 1.f) ? LXF_FILM : -1;
    case TDVC_XF_MASK_LRELU: return LXF_MASK_LRELU;
    case TDVC_XF_MASK_TANH: return LXF_MASK_TANH;
    default: return -1;
  }
}

namespace tdvc { int g_force_generic = 0; }   // test-only switch, like the tdvc_debug_* hooks (misc_kernels.hip)
extern "C" void tdvc_set_force_generic(int on) { g_force_generic = on; }

static Xf to_xf(const tdvc_xform& x) {
  Xf r; r.kind = x.kind; r.slope = x.slope; r.scale = scale_or_1(x.scale);
  r.aux = x.aux; r.aux_bs = x.aux_bs; return r;
}

static int check_desc(const tdvc_conv_desc* d) {
  if (!d) return tdvc_fail(TDVC_EINVAL, "null desc");
  if (d->B <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->Tin <= 0 || d->Tout <= 0 || d->K <= 0 || d->stride <= 0 ||
      d->dilation <= 0 || d->groups <= 0 || d->pad < 0)
    return tdvc_fail(TDVC_EINVAL, "conv desc: non-positive dimension");
  if (d->Cin % d->groups || d->Cout % d->groups) return tdvc_fail(TDVC_EINVAL, "conv desc: channels not divisible by groups");
  if (d->stride > 1 && d->dilation != 1) return tdvc_fail(TDVC_EUNSUPPORTED, "strided conv with dilation");
  if (d->reflect && (d->stride != 1 || d->kind != TDVC_CONV)) return tdvc_fail(TDVC_EUNSUPPORTED, "reflect padding needs stride 1 conv");
  if (d->reflect && d->pad >= d->Tin) return tdvc_fail(TDVC_EINVAL, "reflect padding must be smaller than the input length");
  if (d->w_cin < 0 || d->w_cin_off < 0) return tdvc_fail(TDVC_EINVAL, "conv desc: negative weight channel window");
  if (d->w_cin > 0) {
    if (d->groups != 1 || d->kind != TDVC_CONV) return tdvc_fail(TDVC_EUNSUPPORTED, "weight channel window needs a plain conv with groups == 1");
    if (d->w_cin_off + d->Cin > d->w_cin) return tdvc_fail(TDVC_EINVAL, "conv desc: weight channel window out of range");
  }
  if (d->kind == TDVC_CONV) {
    long expect = ((long)d->Tin + 2L * d->pad - (long)d->dilation * (d->K - 1) - 1) / d->stride + 1;
    if (expect != d->Tout) return tdvc_fail(TDVC_EINVAL, "conv desc: Tout does not match conv arithmetic");
  } else if (d->kind == TDVC_CONV_TRANSPOSE) {
    if (d->stride < 2) return tdvc_fail(TDVC_EUNSUPPORTED, "transposed conv needs stride >= 2");
    long expect = ((long)d->Tin - 1) * d->stride - 2L * d->pad + (d->K - 1) + 1;
    if (d->Tout > expect + d->stride - 1 || d->Tout < expect) return tdvc_fail(TDVC_EINVAL, "conv desc: Tout does not match transposed conv arithmetic");
  } else return tdvc_fail(TDVC_EINVAL, "conv desc: unknown kind");
  return TDVC_OK;
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// What a launch result means to an entry point: TDVC_OK, the recorded TDVC_ELAUNCH or, from a route that may decline
// (hipErrorNotSupported: outside that kernel's contract), TRY_NEXT. TRY_NEXT never leaves this file.
enum { TRY_NEXT = 1 };
static int launch_rc(hipError_t e, bool may_decline = false) {
  if (e == hipSuccess) return TDVC_OK;
  if (may_decline && e == hipErrorNotSupported) return TRY_NEXT;
  return tdvc_fail(TDVC_ELAUNCH, hipGetErrorString(e));
}

// The reduced stride-1 problem of conv_common.h for a pass that writes T columns of R rows per group, reduced over C channels
// per group (GemmConvP and WgradP). The weight strides differ per pass and stay with the caller.
template <class P>
static void set_reduced(P& p, int mode, int R, int C, int T, const tdvc_conv_desc* d) {
  const int s = d->stride;
  p.mode = mode; p.R = R; p.Cred = C; p.N = T; p.J = ceil_div(d->K, s); p.d = 1;
  if (mode == MODE_DIRECT) p.d = d->dilation;                         // s == 1: J = K
  else if (mode == MODE_DOWN) p.Cred = C * s;                         // time-to-depth: s phases per channel
  else { p.R = R * s; p.N = (T - 1 + d->pad) / s + 1; }               // MODE_UP: s output phases per row
}

// Grouped strided conv with 4 -> 4 channels per group (discriminator layer 4): vector-ALU kernels of conv_small_group.hip
static bool small_group_ok(const tdvc_conv_desc* d) {
  return !g_force_generic && g_knob[2] == 0 && d->kind == TDVC_CONV && d->groups >= 16 && d->Cin == 4 * d->groups && d->Cout == 4 * d->groups &&
         d->dilation == 1 && !d->reflect && d->w_cin == 0 && d->stride >= 2 && d->stride <= 8 && d->K <= 48;
}
// Grouped stride-4 conv with 4 -> 16 channels per group (discriminator layers 1-3): forward and input-grad on the MFMA kernels of
// conv_small_group.hip (group16_*). The weight-grad keeps its route. Same off switches as the small-group route.
static bool group16_ok(const tdvc_conv_desc* d) {
  return !g_force_generic && g_knob[2] == 0 && d->kind == TDVC_CONV && d->groups >= 4 && d->Cin == 4 * d->groups && d->Cout == 16 * d->groups &&
         d->stride == 4 && d->K <= 44 && (d->pad & 3) == 0 && d->dilation == 1 && !d->reflect && d->w_cin == 0;
}
static void small_group_base(const tdvc_conv_desc* d, SmallGroupP& q) {
  q.B = d->B; q.G = d->groups; q.Tin = d->Tin; q.Tout = d->Tout; q.K = d->K; q.s = d->stride; q.pad = d->pad;
  q.in_scale = 1.f; q.out_scale = 1.f; q.dy_scale = 1.f;
}

static bool use_mfma(const GemmConvP& p) {
  if (g_force_generic) return false;
  if (p.R <= 2 && p.x.Cg == 1 && p.Cy_g <= 2) return false;   // depthwise / single-channel FIR filters
  return (long)p.Cred * p.J >= 7;                             // Cred is zero-padded to a multiple of 4 in LDS
}

template <int MODE>
static int run_gemm(GemmConvP& p, int B, hipStream_t st) {
  return launch_rc(use_mfma(p) ? launch_conv_gemm<MODE>(p, B, st) : launch_conv_scalar<MODE>(p, B, st));
}

static int dispatch_gemm(GemmConvP& p, int B, hipStream_t st) {
  switch (p.mode) {
    case MODE_DIRECT: return run_gemm<MODE_DIRECT>(p, B, st);
    case MODE_DOWN: return run_gemm<MODE_DOWN>(p, B, st);
    default: return run_gemm<MODE_UP>(p, B, st);
  }
}

// Which kernel a forward or an input-grad call takes, in the order they are tried. The launchers of all but the last may decline.
enum { CV_SMALL_GROUP, CV_GROUP16, CV_LEAN, CV_GENERIC };   // CV_GENERIC: the MFMA or the scalar kernel (use_mfma)

static bool lean_shape_ok(const tdvc_conv_desc* d) {
  return !g_force_generic && d->kind == TDVC_CONV && d->stride == 1 && d->groups == 1 && d->Tin == d->Tout && ((d->Tin & 3) == 0 || d->Tin <= 80);
}

// The lean parameter block of either pass. The caller has put the pass's operands into their roles: q.x, q.w with rows of q.Cw floats,
// q.y, the optional q.res / add / mx / gb / dgb, and Cin / Cout / pad as the kernel sees them (the input-grad reads dy and wt and writes
// dx, channel counts swapped, padding flipped). bs: the batch strides of x, y, res, add, mx, gb, dgb. xf brings the aux operand.
// False: outside the lean kernel's contract (the next route).
static bool lean_fill(const tdvc_conv_desc* d, const tdvc_xform& xf, const long (&bs)[7], LeanP& q, int* xfk) {
  long aux_bs;
  *xfk = lean_xfk(xf, &q.slope, &q.in_scale, &q.aux, &aux_bs);
  const struct { const void* p; long bs; int* q_bs; } opnds[] = {{q.x, bs[0], &q.x_bs}, {q.y, bs[1], &q.y_bs}, {q.res, bs[2], &q.res_bs}, {q.add, bs[3], &q.add_bs},
      {q.mx, bs[4], &q.mx_bs}, {q.gb, bs[5], &q.gb_bs}, {q.dgb, bs[6], &q.dgb_bs}, {q.aux, aux_bs, &q.aux_bs}};
  bool ok = *xfk >= 0 && (q.Cw & 3) == 0 && al16(q.w), vec = (d->Tin & 3) == 0;
  for (const auto& o : opnds) { ok = ok && ok_bs(o.p, o.bs); vec = vec && vec_ptr(o.p, o.bs); *o.q_bs = (int)o.bs; }
  q.T = d->Tin; q.K = d->K; q.d = d->dilation; q.vec = vec ? 1 : 0;
  return ok && (vec || d->Tin <= 80);
}

// First route from `from` on that the descriptor and the call's operands can take. CV_LEAN comes with q and xfk filled.
static int fwd_route(const tdvc_conv_desc* d, const tdvc_conv_fwd_args* a, int from, LeanP& q, int* xfk) {
  if (from <= CV_SMALL_GROUP && small_group_ok(d) && a->x_xf.kind <= TDVC_XF_LRELU && !a->res && !a->add && !a->bias3) return CV_SMALL_GROUP;
  if (from <= CV_GROUP16 && group16_ok(d) && a->x_xf.kind <= TDVC_XF_LRELU && !a->res && !a->add && !a->bias3) return CV_GROUP16;
  if (from <= CV_LEAN && lean_shape_ok(d) && (d->Cin & 3) == 0) {
    q.x = a->x; q.y = a->y; q.bias = a->bias; q.bias3 = a->bias3; q.res = a->res; q.add = a->add;
    q.w = a->w + (long)d->w_cin_off * d->K; q.Cw = (d->w_cin > 0 ? d->w_cin : d->Cin) * d->K;
    q.Cin = d->Cin; q.Cout = d->Cout; q.pad = d->pad; q.reflect = d->reflect;
    q.post = a->post_act; q.out_scale = scale_or_1(a->out_scale); q.add_scale = 1.f; q.m_slope = a->post_slope;
    q.sbits = a->sign_bits; q.sb_bs = (int)a->sign_bits_bs;
    if (lean_fill(d, a->x_xf, {a->x_bs, a->y_bs, a->res_bs, a->add_bs, 0, 0, 0}, q, xfk)) return CV_LEAN;
  }
  return CV_GENERIC;
}

extern "C" int tdvc_conv_fwd(const tdvc_conv_desc* d, const tdvc_conv_fwd_args* a, void* stream) {
  if (int rc = check_desc(d)) return rc;
  if (!a || !a->x || !a->w || !a->y) return tdvc_fail(TDVC_EINVAL, "conv_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  LeanP q = {};
  int xfk = 0, route = CV_SMALL_GROUP;
  while ((route = fwd_route(d, a, route, q, &xfk)) != CV_GENERIC) {
    hipError_t e;
    if (route == CV_SMALL_GROUP || route == CV_GROUP16) {
      SmallGroupP g = {};
      small_group_base(d, g);
      g.x = a->x; g.x_bs = a->x_bs; g.w = a->w; g.bias = a->bias; g.y = a->y; g.y_bs = a->y_bs;
      g.act_in = a->x_xf.kind == TDVC_XF_LRELU; g.slope_in = a->x_xf.slope; g.in_scale = scale_or_1(a->x_xf.scale);
      g.post = a->post_act; g.post_slope = a->post_slope; g.out_scale = scale_or_1(a->out_scale);
      e = route == CV_GROUP16 ? launch_group16_fwd(g, st) : launch_small_group_fwd(g, st);
    } else e = launch_conv_lean(q, d->B, xfk, EPI_FWD, st);
    const int rc = launch_rc(e, true);
    if (rc != TRY_NEXT) return rc;
    ++route;                           // declined: the next route
  }
  // the generic kernels pack no sign bits: only the lean kernel does, inside this contract
  if (a->sign_bits) return tdvc_fail(TDVC_EUNSUPPORTED, "conv_fwd: sign_bits needs a stride-1 conv with Tout % 32 == 0, Tout > 80 and 16-byte aligned operands");
  const int Cin_g = d->Cin / d->groups, Cout_g = d->Cout / d->groups;
  GemmConvP p = {};
  p.x.p = a->x; p.x.bs = a->x_bs; p.x.T = d->Tin; p.x.Cg = Cin_g; p.x.xf = to_xf(a->x_xf);
  p.w = a->w; p.K = d->K; p.s = d->stride; p.pad = d->pad; p.groups = d->groups;
  p.y = a->y; p.y_bs = a->y_bs; p.Ty = d->Tout; p.Cy_g = Cout_g;
  p.epi = EPI_FWD; p.bias = a->bias; p.bias3 = a->bias3; p.res = a->res; p.res_bs = a->res_bs;
  p.post = a->post_act; p.post_slope = a->post_slope; p.out_scale = scale_or_1(a->out_scale);
  p.add = a->add; p.add_bs = a->add_bs; p.add_scale = 1.f;
  p.w_sg = (long)Cout_g * Cin_g * d->K;
  if (d->kind == TDVC_CONV) {
    p.w_sm = (long)Cin_g * d->K; p.w_sc = d->K;
    if (d->w_cin > 0) { p.w_sm = (long)d->w_cin * d->K; p.w += (long)d->w_cin_off * d->K; }
    set_reduced(p, d->stride == 1 ? MODE_DIRECT : MODE_DOWN, Cout_g, Cin_g, d->Tout, d);
    p.reflect = d->reflect;                          // stride 1 only (check_desc)
  } else {
    p.w_sm = d->K; p.w_sc = (long)Cout_g * d->K;
    set_reduced(p, MODE_UP, Cout_g, Cin_g, d->Tout, d);
  }
  return dispatch_gemm(p, d->B, st);
}

static int dgrad_route(const tdvc_conv_desc* d, const tdvc_conv_dgrad_args* a, int from, LeanP& q, int* xfk) {
  if (from <= CV_SMALL_GROUP && small_group_ok(d) && a->epilogue == TDVC_DG_PLAIN && !a->add &&
      (a->dy_xf.kind == TDVC_XF_NONE || (a->dy_xf.kind == TDVC_XF_MASK_LRELU && a->dy_xf.aux))) return CV_SMALL_GROUP;
  if (from <= CV_GROUP16 && group16_ok(d) && a->epilogue == TDVC_DG_PLAIN && !a->add &&
      (a->dy_xf.kind == TDVC_XF_NONE || (a->dy_xf.kind == TDVC_XF_MASK_LRELU && a->dy_xf.aux))) return CV_GROUP16;
  if (from <= CV_LEAN && a->wt && lean_shape_ok(d) && (d->Cout & 3) == 0 && (d->K - 1) * d->dilation - d->pad >= 0) {
    q.x = a->dy; q.y = a->dx; q.add = a->add; q.mx = a->x_in; q.gb = a->gb; q.dgb = a->dgb;
    q.Cw = d->Cout * d->K; q.w = a->wt + (long)d->w_cin_off * q.Cw;       // wt rows: [ci] -> (co, k) contiguous
    q.Cin = d->Cout; q.Cout = d->Cin; q.pad = (d->K - 1) * d->dilation - d->pad; q.flip = 1; q.mirror = d->reflect ? d->pad : 0;
    q.out_scale = 1.f; q.add_scale = a->add_scale; q.m_slope = a->slope;
    if (a->epilogue == TDVC_DG_MASK_LRELU && a->x_sign_bits) { q.mbits = a->x_sign_bits; q.mb_bs = (int)a->x_sign_bits_bs; }
    if (lean_fill(d, a->dy_xf, {a->dy_bs, a->dx_bs, 0, a->add_bs, a->x_in_bs, a->gb_bs, a->dgb_bs}, q, xfk)) return CV_LEAN;
  }
  return CV_GENERIC;
}

extern "C" int tdvc_conv_dgrad(const tdvc_conv_desc* d, const tdvc_conv_dgrad_args* a, void* stream) {
  if (int rc = check_desc(d)) return rc;
  if (!a || !a->dy || !a->w || !a->dx) return tdvc_fail(TDVC_EINVAL, "conv_dgrad: null pointer");
  // the operands each epilogue reads; x_sign_bits may stand in for x_in on the lean route
  if (a->epilogue < TDVC_DG_PLAIN || a->epilogue > TDVC_DG_FILM) return tdvc_fail(TDVC_EINVAL, "conv_dgrad: unknown epilogue");
  const int epi = a->epilogue == TDVC_DG_PLAIN ? EPI_PLAIN : (a->epilogue == TDVC_DG_MASK_LRELU ? EPI_MASK : EPI_FILM);
  if (epi == EPI_MASK && !a->x_in && !a->x_sign_bits) return tdvc_fail(TDVC_EINVAL, "conv_dgrad: mask epilogue needs x_in");
  if (epi == EPI_FILM && (!a->x_in || !a->gb || !a->dgb)) return tdvc_fail(TDVC_EINVAL, "conv_dgrad: FiLM epilogue needs x_in, gb, dgb");
  hipStream_t st = (hipStream_t)stream;
  LeanP q = {};
  int xfk = 0, route = CV_SMALL_GROUP;
  while ((route = dgrad_route(d, a, route, q, &xfk)) != CV_GENERIC) {
    hipError_t e;
    if (route == CV_SMALL_GROUP || route == CV_GROUP16) {
      SmallGroupP g = {};
      small_group_base(d, g);
      g.dy = a->dy; g.dy_bs = a->dy_bs; g.w = a->w; g.y = a->dx; g.y_bs = a->dx_bs;
      g.dy_scale = scale_or_1(a->dy_xf.scale);
      if (a->dy_xf.kind == TDVC_XF_MASK_LRELU) { g.mask = a->dy_xf.aux; g.mask_bs = a->dy_xf.aux_bs; g.m_slope = a->dy_xf.slope; }
      e = route == CV_GROUP16 ? launch_group16_dgrad(g, st) : launch_small_group_dgrad(g, st);
    } else {
      e = launch_conv_lean(q, d->B, xfk, epi, st);
      if (e == hipErrorNotSupported && q.mbits && a->x_in) {   // shape outside the sign-bit path: the fp32 mask source does the same job
        q.mbits = nullptr;
        e = launch_conv_lean(q, d->B, xfk, epi, st);
      }
    }
    const int rc = launch_rc(e, true);
    if (rc != TRY_NEXT) return rc;
    ++route;                           // declined: the next route
  }
  // the generic kernels read no sign bits: only the lean kernel does, inside this contract
  if (epi == EPI_MASK && !a->x_in)
    return tdvc_fail(TDVC_EUNSUPPORTED, "conv_dgrad: x_sign_bits without x_in needs a stride-1 conv with Tin % 32 == 0, Tin > 80 and 16-byte aligned operands");
  const int Cin_g = d->Cin / d->groups, Cout_g = d->Cout / d->groups;
  GemmConvP p = {};
  p.x.p = a->dy; p.x.bs = a->dy_bs; p.x.T = d->Tout; p.x.Cg = Cout_g; p.x.xf = to_xf(a->dy_xf);
  p.w = a->w; p.K = d->K; p.s = d->stride; p.pad = d->pad; p.groups = d->groups;
  p.y = a->dx; p.y_bs = a->dx_bs; p.Ty = d->Tin; p.Cy_g = Cin_g;
  p.add = a->add; p.add_bs = a->add_bs; p.add_scale = a->add_scale;
  p.w_sg = (long)Cout_g * Cin_g * d->K;
  p.epi = epi;
  if (epi != EPI_PLAIN) { p.mx = a->x_in; p.mx_bs = a->x_in_bs; p.m_slope = a->slope; }
  if (epi == EPI_FILM) { p.gb = a->gb; p.gb_bs = a->gb_bs; p.dgb = a->dgb; p.dgb_bs = a->dgb_bs; }
  if (d->kind == TDVC_CONV) {
    p.w_sm = d->K; p.w_sc = (long)Cin_g * d->K;      // rows = input channel, reduced channel = output channel
    if (d->w_cin > 0) { p.w_sc = (long)d->w_cin * d->K; p.w += (long)d->w_cin_off * d->K; }
    set_reduced(p, d->stride == 1 ? MODE_DIRECT : MODE_UP, Cin_g, Cout_g, d->Tin, d);
    if (d->stride == 1) {
      p.tap_flip = 1; p.pad = (d->K - 1) * d->dilation - d->pad;
      if (p.pad < 0) return tdvc_fail(TDVC_EUNSUPPORTED, "conv_dgrad: padding larger than the receptive field");
      p.mirror_pad = d->reflect ? d->pad : 0;
    }
  } else {
    p.w_sm = (long)Cout_g * d->K; p.w_sc = d->K;      // weight [Cin][Cout_g][K] read as a strided conv over dy
    set_reduced(p, MODE_DOWN, Cin_g, Cout_g, d->Tin, d);
  }
  return dispatch_gemm(p, d->B, st);
}

static void fill_wgrad(const tdvc_conv_desc* d, const tdvc_conv_wgrad_args* a, WgradP& p) {
  const int Cin_g = d->Cin / d->groups, Cout_g = d->Cout / d->groups;
  p.groups = d->groups; p.K = d->K; p.s = d->stride; p.pad = d->pad;
  p.w_sg = (long)Cout_g * Cin_g * d->K; p.w_sc = d->K;
  if (d->kind == TDVC_CONV) {
    if (a) { p.a.p = a->dy; p.a.bs = a->dy_bs; p.a.xf = to_xf(a->dy_xf); p.x.p = a->x; p.x.bs = a->x_bs; p.x.xf = to_xf(a->x_xf); }
    p.a.T = d->Tout; p.a.Cg = Cout_g; p.x.T = d->Tin; p.x.Cg = Cin_g;
    p.w_sm = (long)Cin_g * d->K;
    set_reduced(p, d->stride == 1 ? MODE_DIRECT : MODE_DOWN, Cout_g, Cin_g, d->Tout, d);
    p.reflect = d->reflect;                          // stride 1 only (check_desc)
  } else {
    // dW[ci][co][k] = sum_t x[ci][t] * dy[co][t*s - pad + k]: a strided-conv weight-grad with x and dy swapped
    if (a) { p.a.p = a->x; p.a.bs = a->x_bs; p.a.xf = to_xf(a->x_xf); p.x.p = a->dy; p.x.bs = a->dy_bs; p.x.xf = to_xf(a->dy_xf); }
    p.a.T = d->Tin; p.a.Cg = Cin_g; p.x.T = d->Tout; p.x.Cg = Cout_g;
    p.w_sm = (long)Cout_g * d->K;
    set_reduced(p, MODE_DOWN, Cin_g, Cout_g, d->Tin, d);
  }
}

static bool wgrad_use_mfma(const WgradP& p) {
  if (g_force_generic) return false;
  if (p.R <= 2 && p.x.Cg == 1) return false;
  if (!wgrad_mfma_supported(p.J)) return false;
  return true;
}

static bool wgrad_lean_ok(const tdvc_conv_desc* d) {
  const bool wide = d->Cout >= 32 && d->Cin >= 32;     // register-tile kernel: walks (sample, tile) chunks, any length
  return !g_force_generic && d->kind == TDVC_CONV && d->stride == 1 && d->groups == 1 && d->Tin == d->Tout &&
         (d->Tout > 128 || wide) && wgrad_lean_supported(d->Cout, d->Cin, d->K, d->dilation);
}

// split-bf16 weight-grad kernel (conv_wgrad_x6.hip): the layer geometry it takes
static bool wgrad_x6_desc_ok(const tdvc_conv_desc* d) {
  return wgrad_lean_ok(d) && d->w_cin == 0 && wgrad_x6_ok(d->Cout, d->Cin, d->Tout, d->K, d->dilation, d->pad, d->reflect);
}

// Which weight-grad kernel a call takes and what workspace that takes: written once, read by the query and the launch.
enum { WG_SMALL_GROUP, WG_X6, WG_LEAN, WG_MFMA, WG_SCALAR };   // in the order they are tried
struct WgPlan {
  int route;
  int nslab; long sstride;   // slabs left for the fold here and their stride in floats
  bool bias;                 // the slabs carry per-slab bias partials behind the weights
  int bpb;                   // WG_MFMA: samples per block (wgrad_geometry, which also fills p's tile geometry)
  size_t bytes;              // workspace the route needs
};

// First route from `from` on that the descriptor and the call's operands can take; a == null (the workspace query, which
// has no operands to narrow the choice) takes the operand conditions as met.
static WgPlan wgrad_plan(const tdvc_conv_desc* d, const tdvc_conv_wgrad_args* a, WgradP& p, int from) {
  const long wsize = (long)d->groups * p.w_sg;
  WgPlan pl = {};
  auto slabs = [&](int route, int nslab, bool bias) {
    pl.route = route; pl.nslab = nslab; pl.bias = bias; pl.sstride = wsize + (bias ? d->Cout : 0);
    pl.bytes = (size_t)nslab * (size_t)pl.sstride * sizeof(float);
    return pl;
  };
  if (from <= WG_SMALL_GROUP && small_group_ok(d) &&
      (!a || (a->x_xf.kind <= TDVC_XF_LRELU && (a->dy_xf.kind == TDVC_XF_NONE || (a->dy_xf.kind == TDVC_XF_MASK_LRELU && a->dy_xf.aux))))) {
    pl.route = WG_SMALL_GROUP; pl.bias = true; pl.bytes = small_group_wgrad_workspace(d->B, d->groups, d->K);
    return pl;                 // nslab 0: the launcher splits the workspace and folds its slabs, bias partials included, itself
  }
  // 3-tap conv with 65..144 input channels (FiLM cond_var.2): the split-bf16 x6 kernel, dy and x read once per 32-row block
  if (from <= WG_X6 && wgrad_x6_desc_ok(d) &&
      (!a || (a->x_xf.kind <= TDVC_XF_LRELU && a->dy_xf.kind == TDVC_XF_NONE && scale_or_1(a->x_xf.scale) == 1.f && scale_or_1(a->dy_xf.scale) == 1.f &&
              (a->x_xf.kind == TDVC_XF_NONE || (a->x_xf.slope > 0.f && a->x_xf.slope <= 1.f)) &&
              al16(a->x) && al16(a->dy) && (a->x_bs & 3) == 0 && (a->dy_bs & 3) == 0))) {
    int nt, tpb, nslab;
    wgrad_x6_plan(d->Cout, d->Tout, d->B, &nt, &tpb, &nslab);
    return slabs(WG_X6, nslab, true);
  }
  if (from <= WG_LEAN && wgrad_lean_ok(d)) return slabs(WG_LEAN, wgrad_lean_nslab(d->Cout, d->Cin, d->Tout, d->K, d->B), true);
  if (from <= WG_MFMA && wgrad_use_mfma(p)) {
    const int nslab = wgrad_geometry(p, d->B, &pl.bpb);
    return slabs(WG_MFMA, nslab, false);
  }
  pl.route = WG_SCALAR;      // accumulates into dw directly
  return pl;
}

extern "C" size_t tdvc_conv_wgrad_workspace(const tdvc_conv_desc* d) {
  if (check_desc(d)) return 0;
  WgradP p = {};
  fill_wgrad(d, nullptr, p);
  // the largest need of the routes a call can take: the operands pick between small-group and generic, and between x6 and
  // lean. A lean launch that declines is not sized for: its predicate (wgrad_lean_supported) admits no such descriptor.
  size_t need = 0;
  for (int from = WG_SMALL_GROUP; from <= WG_LEAN; ) {
    const WgPlan pl = wgrad_plan(d, nullptr, p, from);
    if (pl.bytes > need) need = pl.bytes;
    from = pl.route + 1;
  }
  return need;
}

extern "C" int tdvc_conv_wgrad(const tdvc_conv_desc* d, const tdvc_conv_wgrad_args* a, void* stream) {
  if (int rc = check_desc(d)) return rc;
  if (!a || !a->x || !a->dy) return tdvc_fail(TDVC_EINVAL, "conv_wgrad: null pointer");
  hipStream_t st = (hipStream_t)stream;
  WgradP p = {};
  fill_wgrad(d, a, p);
  const long wsize = (long)d->groups * p.w_sg;
  // dw rows of the module's weight, or of its w_cin window
  float* dw = (a->dw && d->w_cin > 0) ? a->dw + (long)d->w_cin_off * d->K : a->dw;
  const long dw_rs = d->w_cin > 0 ? (long)d->w_cin * d->K : p.w_sm;
  bool bias_done = false;
  for (int from = WG_SMALL_GROUP; a->dw; ) {
    const WgPlan pl = wgrad_plan(d, a, p, from);
    if (pl.route != WG_SMALL_GROUP && pl.bytes && (!a->workspace || a->workspace_bytes < pl.bytes))   // (the small-group launcher declines instead)
      return tdvc_fail(TDVC_EWORKSPACE, "conv_wgrad: workspace too small");
    hipError_t e;
    if (pl.route == WG_SMALL_GROUP) {
      SmallGroupP q = {};
      small_group_base(d, q);
      q.x = a->x; q.x_bs = a->x_bs; q.dy = a->dy; q.dy_bs = a->dy_bs;
      q.act_in = a->x_xf.kind == TDVC_XF_LRELU; q.slope_in = a->x_xf.slope; q.in_scale = scale_or_1(a->x_xf.scale);
      q.dy_scale = scale_or_1(a->dy_xf.scale);
      if (a->dy_xf.kind == TDVC_XF_MASK_LRELU) { q.mask = a->dy_xf.aux; q.mask_bs = a->dy_xf.aux_bs; q.m_slope = a->dy_xf.slope; }
      e = launch_small_group_wgrad(q, a->dw, a->dbias, a->workspace, a->workspace_bytes, st);
    } else if (pl.route == WG_X6 || pl.route == WG_LEAN) {
      WgLeanP q = {};
      q.a = p.a; q.x = p.x; q.R = d->Cout; q.Cin = d->Cin; q.N = d->Tout; q.pad = d->pad; q.K = d->K; q.reflect = d->reflect;
      q.slab = (float*)a->workspace; q.slab_stride = pl.sstride; q.bias_off = a->dbias ? wsize : -1;
      auto okp = [](const Opnd& o) { return al16(o.p) && (o.bs & 3) == 0 && (o.T & 3) == 0 && (!o.xf.aux || (al16(o.xf.aux) && (o.xf.aux_bs & 3) == 0)); };
      q.vec = (okp(q.a) && okp(q.x)) ? 1 : 0;
      e = pl.route == WG_X6 ? launch_conv_wgrad_x6(q, d->B, st) : launch_conv_wgrad_lean(q, d->B, d->K, d->dilation, st);
    } else if (pl.route == WG_MFMA) {
      p.slab = (float*)a->workspace; p.slab_stride = wsize;
      e = p.mode == MODE_DIRECT ? launch_conv_wgrad<MODE_DIRECT>(p, d->B, pl.bpb, st) : launch_conv_wgrad<MODE_DOWN>(p, d->B, pl.bpb, st);
    } else {
      p.w_sm = dw_rs;
      e = p.mode == MODE_DIRECT ? launch_conv_wgrad_scalar<MODE_DIRECT>(p, d->B, wsize, dw, st)
                                : launch_conv_wgrad_scalar<MODE_DOWN>(p, d->B, wsize, dw, st);
    }
    int rc = launch_rc(e, pl.route == WG_SMALL_GROUP || pl.route == WG_LEAN);
    if (rc == TRY_NEXT) { from = pl.route + 1; continue; }   // declined: the next route
    if (rc == TDVC_OK && pl.nslab)       // compact slab rows [Cin_g*K] -> dw rows; bias partials, where carried, -> dbias
      rc = launch_rc(launch_slab_reduce((const float*)a->workspace, pl.nslab, pl.sstride, pl.bias && a->dbias ? pl.sstride : wsize, dw, (int)p.w_sm, dw_rs,
                                        st, wsize, pl.bias ? a->dbias : nullptr));
    if (rc) return rc;
    bias_done = pl.bias;
    break;
  }
  if (a->dbias && !bias_done) {
    Opnd dy; dy.p = a->dy; dy.bs = a->dy_bs; dy.T = d->Tout; dy.Cg = d->Cout / d->groups; dy.xf = to_xf(a->dy_xf);
    return launch_rc(launch_bias_grad(dy, d->Tout, d->Cout, d->B, a->dbias, st));
  }
  return TDVC_OK;
}


// FiLM conditioning forward (model/generator.py:86-92,103-104): gb = cond_var.2(LeakyReLU(cond_var.0(c))), where
// cond_var.0 is evaluated as [time-constant speaker part = k3] + [n_var-channel excitation window of its weight].
extern "C" int tdvc_film_cond_fwd(const tdvc_film_cond_args* a, void* stream) {
  if (!a || !a->exc || !a->w0 || !a->k3 || !a->w2 || !a->gb) return tdvc_fail(TDVC_EINVAL, "film_cond_fwd: null pointer");
  if (a->B <= 0 || a->T < 4 || a->n_cond <= a->n_var || a->n_var <= 0 || a->C2 <= 0) return tdvc_fail(TDVC_EINVAL, "film_cond_fwd: bad shape");
  LeanP q = {};
  q.x = a->exc; q.x_bs = (int)a->exc_bs; q.w = a->w2; q.bias = a->b2; q.y = a->gb; q.y_bs = (int)a->gb_bs;
  q.T = a->T; q.Cin = a->n_cond; q.Cout = a->C2; q.Cw = a->n_cond * 3; q.K = 3; q.d = 1; q.pad = 1;
  q.cw = a->w0 + (long)(a->n_cond - a->n_var) * 3; q.cw_stride = a->n_cond * 3; q.Cv = a->n_var;
  q.k3 = a->k3; q.cv0 = a->cv0; q.cv0_bs = (int)a->cv0_bs;
  q.slope = a->slope; q.in_scale = 1.f; q.out_scale = 1.f; q.add_scale = 1.f; q.m_slope = a->slope; q.post = TDVC_POST_NONE;
  q.vec = ((a->T & 3) == 0 && vec_ptr(a->gb, a->gb_bs) && vec_ptr(a->cv0, a->cv0_bs) && al16(a->w2) && ((a->n_cond * 3) & 3) == 0) ? 1 : 0;
  hipError_t e = launch_conv_lean_cond(q, a->B, (hipStream_t)stream);
  if (e == hipErrorNotSupported) return tdvc_fail(TDVC_EUNSUPPORTED, "film_cond_fwd: shape outside the fused kernel's contract");
  return e == hipSuccess ? TDVC_OK : tdvc_fail(TDVC_ELAUNCH, hipGetErrorString(e));
}

// Deferred weight-gradient folds (include/tdvc.h)
extern "C" void tdvc_fold_defer(int on) { tdvc::fold_set_defer(on); }
extern "C" void tdvc_fold_reset(void* stream) { tdvc::fold_reset((hipStream_t)stream); }
extern "C" int tdvc_fold_flush(void* stream) { return launch_rc(tdvc::fold_flush((hipStream_t)stream)); }
// Test and tool access to the fold kernel (include/tdvc.h)
extern "C" int tdvc_debug_slab_fold(const float* slab, int32_t nslab, int64_t stride, int64_t n, float* dw, int32_t rowlen, int64_t dst_row_stride,
                                    int64_t n_w, float* dbias, int32_t ref, void* stream) {
  if (n_w < 0) n_w = n;
  if (!slab || !dw || nslab < 1 || n < 1 || stride < n || n_w > n || rowlen < 1 || dst_row_stride < rowlen || (n_w < n && !dbias))
    return tdvc_fail(TDVC_EINVAL, "debug_slab_fold: bad arguments");
  return launch_rc(tdvc::debug_slab_fold(slab, nslab, stride, n, dw, rowlen, dst_row_stride, n_w, dbias, ref, (hipStream_t)stream));
}
extern "C" void tdvc_debug_fold_log(int on) { tdvc::fold_log_set(on); }
extern "C" size_t tdvc_debug_fold_log_read(double* rows, size_t cap_rows) { return tdvc::fold_log_read(rows, cap_rows); }
