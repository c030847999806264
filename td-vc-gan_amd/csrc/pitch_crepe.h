// What the CREPE forward (pitch_crepe.hip) and backward (pitch_crepe_bwd.hip) kernels share: the geometry constants of the network
// and of the implicit-GEMM tile, one definition each.
#pragma once
#include <hip/hip_runtime.h>

namespace tdvc {

constexpr int CR_WIN = 1024, CR_BINS = 360, CR_THREADS = 256;
constexpr int CR_KCH = 128;          // products per chunk and chain (K 64 geometry, and the forward of layer 1)
constexpr int CR_WP = 130;           // ws row pitch for CR_KCH products: 2 mod 32
constexpr int CR_L1_U = 136;         // layer-1 backward: taps-per-position offsets u in [-64, 72), 132 of them live (see pitch_crepe_bwd.hip)
constexpr int CR_L1_WP = 162;        // ws row pitch for CR_L1_U products: 2 mod 32

typedef float cr_f32x4 __attribute__((ext_vector_type(4)));

// the pooling decision of one output (include/tdvc.h, tdvc_crepe_conv_train)
enum : unsigned char { CR_CODE_DEAD = 0, CR_CODE_EVEN = 1, CR_CODE_ODD = 2 };

}  // namespace tdvc
