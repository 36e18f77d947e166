// Winograd / Toom-Cook F(4,5) form of the post-net's three 512 -> 512 Conv1d layers (5 taps, stride 1, pad 2): four outputs of one channel pair from
// 8 multiplications instead of 20.  Points {0, 1, -1, 2, -2, 1/2, -1/2, inf}.  For a tile d[0..7] = x[4j - 2 .. 4j + 5] and taps g[0..4]
//      y[4j + i] = sum_k g[k] d[i + k] = sum_p AT[i][p] (G g)[p] (BT d)[p],   i = 0..3
// and over the input channels the eight point-wise products become eight GEMMs of K = 512 (one grouped launch of the split-bf16 family):
//      V_p = BT d (post_wino_in) -> M_p = V_p U_p^T -> y = AT M (post_wino_out, with the layer's scale / shift, PSine and residual).
// AT and BT are dyadic (exact in fp32; the transforms apply them in fp32, in one fixed order); G is not: U_p = sum_k G[p][k] W[:, :, k] is formed in fp64,
// rounded once to fp32 (post_wino_weights), and its bf16 planes are the exact split of that fp32 matrix.
#pragma once
#include "l2s_common.h"

namespace l2s {

constexpr int WINO_P = 8, WINO_M = 4, WINO_R = 5;      // points, outputs per tile, taps
constexpr double WINO_AT[WINO_M][WINO_P] = {
    {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0},
    {0.0, 1.0, -1.0, 2.0, -2.0, 1.0 / 2.0, -1.0 / 2.0, 0.0},
    {0.0, 1.0, 1.0, 4.0, 4.0, 1.0 / 4.0, 1.0 / 4.0, 0.0},
    {0.0, 1.0, -1.0, 8.0, -8.0, 1.0 / 8.0, -1.0 / 8.0, 1.0}};
constexpr double WINO_G[WINO_P][WINO_R] = {
    {-1.0, 0.0, 0.0, 0.0, 0.0},
    {-2.0 / 9.0, -2.0 / 9.0, -2.0 / 9.0, -2.0 / 9.0, -2.0 / 9.0},
    {-2.0 / 9.0, 2.0 / 9.0, -2.0 / 9.0, 2.0 / 9.0, -2.0 / 9.0},
    {1.0 / 90.0, 1.0 / 45.0, 2.0 / 45.0, 4.0 / 45.0, 8.0 / 45.0},
    {1.0 / 90.0, -1.0 / 45.0, 2.0 / 45.0, -4.0 / 45.0, 8.0 / 45.0},
    {32.0 / 45.0, 16.0 / 45.0, 8.0 / 45.0, 4.0 / 45.0, 2.0 / 45.0},
    {32.0 / 45.0, -16.0 / 45.0, 8.0 / 45.0, -4.0 / 45.0, 2.0 / 45.0},
    {0.0, 0.0, 0.0, 0.0, 1.0}};
constexpr double WINO_BT[WINO_P][WINO_P] = {
    {-1.0, 0.0, 21.0 / 4.0, 0.0, -21.0 / 4.0, 0.0, 1.0, 0.0},
    {0.0, 1.0, 1.0, -17.0 / 4.0, -17.0 / 4.0, 1.0, 1.0, 0.0},
    {0.0, -1.0, 1.0, 17.0 / 4.0, -17.0 / 4.0, -1.0, 1.0, 0.0},
    {0.0, 1.0 / 2.0, 1.0 / 4.0, -5.0 / 2.0, -5.0 / 4.0, 2.0, 1.0, 0.0},
    {0.0, -1.0 / 2.0, 1.0 / 4.0, 5.0 / 2.0, -5.0 / 4.0, -2.0, 1.0, 0.0},
    {0.0, 2.0, 4.0, -5.0 / 2.0, -5.0, 1.0 / 2.0, 1.0, 0.0},
    {0.0, -2.0, 4.0, 5.0 / 2.0, -5.0, -1.0 / 2.0, 1.0, 0.0},
    {0.0, -1.0, 0.0, 21.0 / 4.0, 0.0, -21.0 / 4.0, 0.0, 1.0}};

inline int wino_tiles(int S) { return (S + WINO_M - 1) / WINO_M; }      // tiles of one clip: every clip has its own tile grid from its own t = 0
// one layer's transformed weights: U [8 points][C][C] fp32, then the eight matrices' bf16 planes (gemm_planes_bytes(C, C) each)
int64_t wino_weights_bytes(int C);
inline const float* wino_u(const void* base, int C, int p) { return reinterpret_cast<const float*>(base) + (int64_t)p * C * C; }
inline const void* wino_u3(const void* base, int C, int p) {
    return reinterpret_cast<const char*>(base) + (int64_t)WINO_P * C * C * 4 + p * gemm_planes_bytes(C, C);
}
// W: the packed Conv1d weight [C][5 * C] (k = tap * C + ci) -> out (wino_weights_bytes(C))
int launch_post_wino_weights(const float* W, int C, void* out, hipStream_t s);
// x (B, S, C) -> V [8][B * wino_tiles(S)][C]; frames outside [0, S) read as zeros
int launch_post_wino_in(const float* x, int B, int S, int C, float* V, hipStream_t s);
// M [8][B * wino_tiles(S)][C] -> y (B, S, C) = PSine(AT M * scale + shift) + resid; rows past S are dropped
int launch_post_wino_out(const float* M, int B, int S, int C, const float* scale, const float* shift, const float* actw, const float* resid, float* y, hipStream_t s);

}  // namespace l2s
