// daco_gnn.h -- the heuristic network's parameter block, shared by the inference kernels (daco_gnn.hip) and the training
// kernels (daco_gnn_train.hip, whose gradient block has the same layout).
#pragma once
#include "daco_device.h"

namespace daco {

// ---- parameter block layout (floats), built by the host (deepaco_amd/net.py pack_params)
// [0]               v_lin0.W [32][feats] | v_lin0.b [32]
// then              e_lin0.W [32]        | e_lin0.b [32]
// then 12 x layer:  WvT [32 c][128 c']  (x1|x2|x3|x4 outputs, transposed) | bv [128]
//                   We [32 o][32 c] | be [32] | bn_v scale[32] shift[32] | bn_e scale[32] shift[32]
// then head:        W1 [32][32] b1 [32] W2 [32][32] b2 [32] W3 [32] b3 [1]
constexpr int LAYER_FLOATS = 32 * 128 + 128 + 32 * 32 + 32 + 4 * 32;
__host__ __device__ inline size_t off_layer(int feats, int l) { return (size_t)32 * feats + 32 + 64 + (size_t)l * LAYER_FLOATS; }
__host__ __device__ inline size_t off_head(int feats) { return off_layer(feats, 12); }
constexpr int HEAD_FLOATS = 2 * (32 * 32 + 32) + 32 + 1;

// row of a 32 x 32 MFMA output tile that accumulator register r of `lane` holds
__device__ inline int drow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

}  // namespace daco
