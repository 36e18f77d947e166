// Internal declarations shared by the HIP translation units of libl2s_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#define L2S_WAVE 64

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct l2s_resize_job;      // include/l2s.h
struct l2s_align_job;
#ifdef L2S_DIAG
struct l2s_gemm_bwd_record; // include/l2s_diag.h
#endif

namespace l2s {

// ---------------------------------------------------------------- error handling
void set_error(const std::string& msg);
#define L2S_CHECK_HIP(expr)                                                                   \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            l2s::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)
#define L2S_REQUIRE(cond, msg)                                                                \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            l2s::set_error(std::string("l2s: ") + (msg) + " [" #cond "]");                    \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

// ---------------------------------------------------------------- optional per-kernel event timing
void prof_begin(const char* name, hipStream_t s);
void prof_end(hipStream_t s);
void prof_count(const char* name, int64_t n);      // a counter among the profile entries: adds n to its `launches` (no time); nothing when profiling is off
struct ProfScope {
    hipStream_t s;
    ProfScope(const char* name, hipStream_t st) : s(st) { prof_begin(name, st); }
    ~ProfScope() { prof_end(s); }
};

// ---------------------------------------------------------------- run-time options (include/l2s.h "run-time options")
// Every model carries its own copy (l2s_model::opt, copied from the process defaults at l2s_model_create), so host threads that drive
// different models - or one model - never read a switch another thread is flipping.
struct Options {
    int fold = 1;               // "fold_step_weights": phase-merged 4-launch step vs the literal 6-phase step
    int graph = 0;              // "use_graph": replay the decode loop from a captured hipGraph
    int overlap_postnet = 0;    // "overlap_postnet": windowed post-net on a second stream under the decode loop
    int fuse_trunk = 1;         // "fuse_trunk": stride-1 ShuffleNet units as one fused kernel each
    int fuse_s2 = 1;            // "fuse_s2": stride-2 ShuffleNet units as one fused kernel each (needs fuse_trunk)
    int trunk_x3 = 1;           // "trunk_x3": the fused units' pointwise convs on the bf16 matrix cores through the exact three-way split (activations split once where
                                //             they are written to LDS, weights as pre-split operand planes); 0 = the f32-MFMA units
    int refresh_map = 0;        // "refresh_map": l2s_model_finalize also builds the device-side refresh map (training)
    int skinny_static = 0;      // "skinny_static": compile-time K-segment layouts in the batch-row kernels
    int skinny_sized = 1;       // "skinny_sized": batch-row instances sized for the launch's longest K
    int skinny_split = 2;       // "skinny_split": operand-load batches of the K <= 1536 instance
    int skinny_split8 = 1;      // "skinny_split8": the same for the K <= 1024 instance
    int rc_shape = 0;           // "skinny_rc": register-blocked batch-row blocks for >= 64 rows: 0 = by tile count, 11 = never, 21 / 22 / 42 = force RT x CT
    int rc_jb = 0;              // "skinny_rc_jb": operand batching of the register-blocked blocks: 0 = 4x2 blocks one chunk per batch and four batches in flight, smaller shapes two chunks per batch and two in flight; 2 / 4 = that many chunks per batch, two in flight, every shape; 15 = 4x2 with five in flight
    int gemm_x3_dma = 1;        // "gemm_x3_dma": constant Conv1d / Linear weights of the split-bf16 GEMMs as pre-split planes fetched by LDS-DMA (ConvW::W3)
    int lstm_x3 = 4;            // "lstm_x3": the decode step's LSTM launches on the bf16 matrix cores (exact three-way split, pre-split weight planes): 2 = eight-wave
                                //   blocks, 1 = four-wave blocks, 3 = as 2, but the 4x2 blocks (>= 192 rows) as four-wave blocks of at most 256 registers - half
                                //   a compute unit, so that kernels of other launch chains run beside them (all the same bits), 0 = the f32 MFMA form;
                                //   4 (default) = as 3, but the K = 1024 launches (the step's two) as ONE eight-wave block per CU of 64 rows x 64 gate columns
                                //   whose two column halves share one activation panel through LDS (skinny_block_sp); every other launch as 3.  Same bits
    int half_min_mts = 12;      // "half_min_mts": with "lstm_x3" >= 3 and chains overlapping, an LSTM launch takes the half-CU 4x2 form (or the shared-panel form) from this many 16-row tiles
                                //   on (13: where 4x2 blocks give >= 224 blocks anyway; 12: also the 192-row launches of a six-batch group, whose 384 2x2
                                //   eight-wave blocks otherwise fill every CU for two rounds - the driver's 20-step command cuts into 7 + 7 + 6 batches:
                                //   3.14-3.18 -> 3.21-3.29 M in three A/B pairs; 8: no better there, worse at 128 / 160 rows); same bits
    int flat_half = 1;          // "flat_half": the flat first phase of the step on four-wave 2x1 / 2x2 blocks (at most 153 registers, 39 KB of LDS: two or
                                //   three per CU, up to 512 per launch) instead of eight-wave blocks that sit alone on their CU - so that other chains'
                                //   kernels run beside them; same bits
    int attn_lds = 1;           // "attn_lds": the step's attention blocks fetch keys / projected values by buffer loads, the values as 16-byte rows through LDS:
                                //   1 = at up to 128 rows per launch, 2 = always, 0 = never
    int hoist_vproj = 3;        // "hoist_vproj": the phase-merged step reads o = a @ V' with V' = V W_ap^T + b_ap computed once in the prologue: 3 (default) = as 2,
                                //   and the content columns leave the step too: LSTM0 on [prenet + o | h0] (K = 768), W_ih[:, content] (alpha @ value) added by the
                                //   cell threads as sum_j alpha_j P_j with P = value W_ih[:, content]^T from the prologue (clips of at most CONTENT_HOIST_MAX_M
                                //   content slots; longer clips run 2, same bits as 2), 2 = LSTM0 on
                                //   [content | prenet + o | h0] (K = 1024, the sum formed by the operand loader: the reference's own u = prenet + o), 1 = on
                                //   [content | prenet | o | h0] through a second copy of W_ih's u columns (K = 1280; every block form), 0 = a @ v through the
                                //   pre-multiplied W_ih W_ap (K = 1536)
    int skinny_flat = 1;        // "skinny_flat": launches with several GEMM groups at >= 64 rows run per-group block shapes in one flat grid of at most one
                                //   block per CU (the step's first phase), instead of one block shape for every group
    int rc_shape_multi = 0;     // "skinny_rc_multi": the same choice for launches that carry several GEMM groups (the step's first phase); 0 = as "skinny_rc"
    int gemm_x3 = 1;            // "gemm_x3": inference GEMMs / Conv1d stacks on the split-bf16 kernel (gemm_x3.hip) where eligible; 5 = its 128x128x32 tile only
    int frontend_x3 = 3;        // "frontend_x3": the inference front-end conv on the split-bf16 matrix path (frontend3d_x3_kernel); 2: its two-output-frames-per-block
                                //   form (frontend3d_x3p_kernel); 3 (default): the same with the next slab's staging interleaved between the MFMA groups of the
                                //   current one (frontend3d_x3q_kernel: double-buffered input planes, one barrier per slab; same bits: 0.593 -> 0.562 ms at 32 clips,
                                //   1.907 -> 1.832 at 128, 3.61 -> 3.59 at 256 - at 256 clips the kernel sits at the chip's clock under MFMA load)
    int train_bf16 = 0;         // "train_bf16": the training step's GEMMs / Conv1d stacks (forward and backward) with bf16 operands on the bf16 matrix cores
    int persist = 4;            // "persist_decode": the free-running decode loop of a single-batch call with at most this many clips (pdecode.hip: up to 4 clips
                                //   of <= 32 frames - "persist_frames" below: up to 80 -, two per launch) as persistent weight-stationary launches instead of four launches per step; 0 = never.  A
                                //   latency form: one call owns the chip, such launches are chained one after the other; grouped calls (l2s_*_multi) never take it
    int persist_frames = 32;    // "persist_frames": the longest clip (frames) whose calls take the persistent forms; above 32 the long-clip forms of the decode loop
                                //   (pdecode.hip: two key frames per thread in registers, the keys of up to 16 more frames in LDS) serve clips of up to 80 frames.
                                //   Values below 32 act as 32 (the short forms are "persist_decode"'s), values above 80 as 80; the default changes nothing
    int persist_masked = 0;     // "persist_masked": > 0 = free-running masked calls (per-clip video lengths) inside the envelope of the two options above take the
                                //   persistent forms too (pdecode.hip: the length-masked instantiations - a clip's workgroups run the loop of its own length; the
                                //   prologue's BiLSTM at <= 2 clips); 0 (default) = masked calls always take the launch-per-phase route
    int frontend_solo = 0;      // "frontend_solo" (diagnostic A/B): when chains overlap, the front-end conv takes ONE block per CU (an LDS pad) so that step kernels of other
                                //   chains (half-CU blocks) run beside it instead of waiting for its 530-us blocks to retire
    int trunk_chain = 1;        // "trunk_chain" (diagnostic A/B): the consecutive stride-1 units of a ShuffleNet stage as ONE launch (the map stays on chip between the
                                //   units; stages 2 and 3 - at 3x3 the per-unit launches are 5 % faster): 3 + 7 launches become 2, the trunk 3.82 -> 3.52 ms per 256 clips,
                                //   same bits; 0 = one launch per unit, 2 = the 3x3 stage as well
    int flat_xcd = 1;           // "flat_xcd" (diagnostic A/B): the flat first phase's block -> tile map XCD-affine (an XCD = one row half x one column quarter of a group:
                                //   weights through two L2s, activations through four, instead of one and eight): 22.3 -> 18.4 MB through the fabric per launch; same bits
    int attn_skip0 = 1;         // "attn_skip0" (diagnostic A/B): when chains overlap, the attention blocks fetch a frame's projected values only if its soft-max weight is
                                //   not exactly zero (28.4 -> 23.5 MB per launch; same bits); 2 = also for a chain alone (one more round trip in the block: slower there), 0 = never
    int early_stop = 0;         // "early_stop": free-running inference ends the decode loop once every clip of the call has crossed its stop token, plus the post-net's
                                //   receptive margin (ES_MARGIN steps); frames at or past a clip's length come back as exact zeros (include/l2s.h)
    int post_wino = 1;          // "post_wino" (diagnostic A/B): post-net layers 1-3 in their Winograd F(4,5) form (post_wino.h: eight K = 512 products per layer in place of
                                //   one K = 2560 product, 0.4x the matrix work; another association of the same sums): 1 = on the plain full-range route from
                                //   POST_WINO_ROWS rows per batch on, 2 = at any row count, 0 = never.  The tap-split and windowed routes, "infer_bf16", "gemm_x3" = 0 and
                                //   training keep the direct layer
    int infer_bf16 = 0;         // "infer_bf16": the bf16 leg of inference / evaluate: front-end conv, GEMMs and Conv1d stacks of encoder, prologue, post-net and
                                //   voice tower with bf16 operands (fp32 accumulation); the recurrent loops, the fused ShuffleNet units and all statistics stay fp32
};
int set_option_field(Options& o, const char* name, int value);    // 0 = ok, 1 = unknown name

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_SILU = 2, ACT_PSINE = 3, ACT_PRELU = 4 /* backward only */ };

// ---------------------------------------------------------------- tiled fp32 MFMA GEMM (gemm_nt.hip)
// C[m, n] = epilogue( sum_k A(m,k) * W[n*K + k] ), A addressed as an implicit Conv1d over channel-last
// sequences: row m = (b, t), k = (tap, ci), element X[(b*Tin + t*stride + tap - pad) * lda + col(ci)].
struct GemmP {
    const float* A;
    const float* W;       // [N][K], K contiguous, k = tap*Cin + ci
    const float* scale;   // [N] or null (1)
    const float* shift;   // [N] or null (0)     v = acc*scale + shift
    const float* actw;    // [N] for ACT_PSINE
    const float* R1;      // optional addend after the activation: R1[(r1_mod ? m % r1_mod : m)*ldr1 + n]
    const float* R2;
    float* C;
    int M, N, K;
    int lda, Tout, Tin, taps, stride, pad, Cin;
    int a_split, a_gap;   // channel ci >= a_split reads column ci + a_gap (two-segment A rows)
    int act;
    int ldr1, r1_mod, ldr2, r2_mod;
    int r2_div;           // > 0: R2 row index = m / r2_div (a per-sequence row broadcast over its time steps)
    int ldc, c_cstride;   // C[m*ldc + n*c_cstride]
    int c_tr_T;           // > 0: C[((m / T)*N + n)*T + m % T]  (channel-first store per sequence)
    float* Zout;          // training: pre-activation value (after scale/shift), same addressing as C (row-major form only)
    int win_T, win_off;   // win_T > 0: rows cover the time window [win_off, win_off + Tout) of sequences of length win_T:
                          //   input frame = (win_off + t)*stride + tap - pad, output/residual row = b*win_T + win_off + t
    int vec;              // 4: float4 operand loads (K, Cin, lda, offsets multiples of 4); 1: scalar loads
    const float* mask;    // training: dropout multiplier mask[m*ldmask + n], applied after activation and addends
    int ldmask, mask_pre; //   (mask_pre: after the activation, before the addends)
    int ldw;              // row stride of W in floats (0: K) - a K slice of a wider matrix (split-K)
    const void* W3;       // W as pre-split bf16 planes [ceil32(K) / 16][3 planes][N][16 k], zeros past K (launch_gemm_planes; N % 256 == 0, K % 16 == 0, ldw == 0) or null: the
                          //   128x256x32 split-bf16 tile then brings its weight operand in by LDS-DMA instead of load + split + ds_write
    int x3;               // bit 1: run on the split-bf16 kernel (gemm_x3.hip) when the whole launch group is eligible; bit 2: whatever its size
                          //   (operator tests); bit 4: the 128x128x32 tile only; set from gemm_x3_mode(); bit 8: always the split-bf16 family, the tile by
                          //   the usual cost rule (the post-net's Winograd products: no row threshold may hand them to the f32 kernel)
    int x3_group;         // batches sharing this launch (grouped inference): the size thresholds of the kernel choice look at M / x3_group,
                          //   so a batch meets the same kernels alone and in a group (results stay bit-identical)
    float* stats;         // training, batch-statistics BatchNorm: STATS PASS - nothing is stored; per-column sums of the raw product
                          //   (no scale/shift) go to stats[(blockIdx.y*2 + {0: sum, 1: sum of squares})*N + n]
    int stats_raw;        // STATS PASS with stats_raw: the raw product is also parked at the Zout addresses, and launch_gemm_finish runs the
                          //   epilogue over it once this batch's scale/shift exist - ONE pass over the product instead of two
};
inline int64_t gemm_stats_floats(int M, int N) { return (int64_t)((M + 63) / 64) * 2 * N; }
constexpr int GEMM_MAX_GROUP = 8;
struct GemmBatch {
    GemmP p[GEMM_MAX_GROUP];
    int count;
};
GemmP gemm_plain(const float* A, int lda, const float* W, float* C, int ldc, int M, int N, int K);
// split-bf16 GEMM (gemm_x3.hip): fp32 operands split into 3 bf16 planes on their way into LDS, six bf16 MFMAs per K step instead of the
// f32 MFMA chain.  gemm_plain() stamps new descriptors with the calling thread's current mode; the inference launch sequences open an
// X3Scope with their model's "gemm_x3" option, everything else (training, operator tests) stays on the f32 kernel unless it asks.
int& gemm_x3_mode();                     // thread-local
int& gemm_x3_group();                    // thread-local: batches per launch chain (1 outside l2s_inference_multi)
struct X3Scope { int prev; explicit X3Scope(int on) : prev(gemm_x3_mode()) { gemm_x3_mode() = on; } ~X3Scope() { gemm_x3_mode() = prev; } };
int& chains_hint();                     // thread-local: launch chains the CALLER keeps in flight on the device (l2s_set_thread_chains; 1 = this thread's calls have the chip to themselves)
bool& grouped_entry();                  // thread-local: inside an l2s_*_multi call, whatever G (such calls never take the persistent latency forms)
struct X3Group {
    int prev; bool prev_grouped;
    explicit X3Group(int g) : prev(gemm_x3_group()), prev_grouped(grouped_entry()) { gemm_x3_group() = g; grouped_entry() = true; }
    ~X3Group() { gemm_x3_group() = prev; grouped_entry() = prev_grouped; }
};
// bf16-operand mode of the TRAINING GEMMs (forward gemm_nt.hip and backward gemm_bwd.hip; option "train_bf16"): operands rounded to bf16
// (RNE) while they are staged into LDS, v_mfma_f32_32x32x16_bf16, fp32 accumulation, fp32 results.  Thread-local, opened by the l2s_train_*
// entry points; the recurrent loop, the front-end conv, BatchNorm statistics and every elementwise kernel stay fp32.
int& gemm_bf16_mode();
struct Bf16Scope { int prev; explicit Bf16Scope(int on) : prev(gemm_bf16_mode()) { gemm_bf16_mode() = on; } ~Bf16Scope() { gemm_bf16_mode() = prev; } };
bool gemm_x3_eligible(const GemmBatch& b);
bool gemm_x3_member_ok(const GemmP& p);               // one member's operands and shape (no launch-size threshold)
int64_t gemm_planes_bytes(int N, int K);                                                // N * ceil32(K) * 6
int launch_gemm_planes(const float* W, int N, int K, void* planes, hipStream_t s);      // planes: gemm_planes_bytes(N, K)
int launch_gemm_x3(const GemmBatch& b, hipStream_t s, const char* name);
void gemm_x3_set_timeline(unsigned long long* ts, int block);      // non-null: launch the stamped measurement build (tools/gemm_x3_timeline.py)
// split-K for plain GEMMs whose 64x64 tiles are too few to fill the chip (M <= 128 rows in the content path, the B-row Linears):
// <= 8 K slices as ONE grouped launch writing raw partial products to part[slice][M][N], then one kernel that adds the slices in
// order and runs the usual epilogue of `p`. Deterministic. part: ksplit*M*N floats.
int launch_gemm_splitk(const GemmP& p, int ksplit, float* part, hipStream_t s, const char* name);
int launch_gemm_splitk_group(const GemmBatch& g, int ksplit, float* part, hipStream_t s, const char* name);   // count*ksplit <= 8; part: count*ksplit*M*N
// the same for a group of Conv1d layers whose tile counts are small and whose K = taps*Cin is long (Content.agg: 2-15 row tiles,
// K up to 3584): one K slice per TAP (a 1-tap conv with a shifted pad), all slices of all layers in grouped launches, then one finish
// kernel per multi-tap layer. part: sum over the multi-tap layers of taps*M*N floats.
int launch_gemm_tapsplit(const GemmBatch& convs, float* part, hipStream_t s, const char* name);
int launch_gemm(const GemmBatch& b, hipStream_t s, const char* name);
// train() mode, convs in front of a batch-statistics BatchNorm: after a stats pass with stats_raw = 1 (and bn_stats_finalize), the fused epilogue
// of `b` (scale/shift, Zout, activation, masks, addends, any store form) element by element over the parked raw products - the same gemm_store
// on the same accumulator values as a second GEMM pass, bit for bit, for an M x N elementwise pass instead of the product
int launch_gemm_finish(const GemmBatch& b, hipStream_t s, const char* name);
int launch_gemm1(const GemmP& p, hipStream_t s, const char* name);

// ---------------------------------------------------------------- backward GEMMs (gemm_bwd.hip)
enum BwdMode { BWD_DX = 0, BWD_DW = 1 };
struct BwdGemmP {
    int mode;
    const float* A; int lda;     // dZ
    const float* B; int ldb;     // DX: forward-layout weight [Nout][taps*Cin];  DW: forward input X (B,Tx,Cin)
    float* C; int ldc;           // DX: dX;  DW: dWp [Nout][taps*Cin]
    int M, N, K;                 // C is M x N, reduction length K
    int Tx, Tz, taps, stride, pad, padp, Nout, Cin;
    int c_T; int64_t c_seq_stride;   // c_T > 0: C row = (m / c_T) * c_seq_stride + (m % c_T) * ldc
    float alpha; int accumulate;
    int vec;                     // set by launch_gemm_bwd: operands allow 16-byte loads
    int ksplit; int64_t c_split_stride;   // DW: reduction split over gridDim.z into partial matrices (launch_gemm_bwd_splitk)
};
BwdGemmP bwd_dx(const float* dZ, int ldz, const float* Wp, float* dX, int ldx, int B, int Tz, int Tx, int Nout, int Cin, int taps, int pad, bool accumulate);
BwdGemmP bwd_dw(const float* dZ, int ldz, const float* X, int ldx, float* dWp, int B, int Tz, int Tx, int Nout, int Cin, int taps, int stride, int pad, bool accumulate);
int launch_gemm_bwd(const BwdGemmP& p, hipStream_t s, const char* name);
int64_t gemm_bwd_splitk_floats(const BwdGemmP& p, int splits);
int launch_gemm_bwd_splitk(const BwdGemmP& p, int splits, float* partials, hipStream_t s, const char* name);
// weight gradient (split-K as above) and input gradient of one 1x1 layer in ONE launch (they share dZ and are independent)
int launch_gemm_bwd_dw_dx(const BwdGemmP& pdw, int splits, float* partials, const BwdGemmP& pdx, hipStream_t s, const char* name);
#ifdef L2S_DIAG      // launch recorder of the three functions above (include/l2s_diag.h l2s_gemm_bwd_record): host code of libl2s_diag.so only
const ::l2s_gemm_bwd_record& gemm_bwd_last_record();      // what the calling thread's last launch ran; zeroes after gemm_bwd_clear_last_record
void gemm_bwd_clear_last_record();
int gemm_bwd_recorder(int cmd, ::l2s_gemm_bwd_record* out, int cap, int* count);
#endif

// Backward of a fused GEMM epilogue  y = act(z) [+ residual],  z = conv * s + shift  (s, shift = eval-mode BatchNorm and/or bias):
//   dpre = dy * act'(z);  dconv = dpre * s;  per-column sums  r0 = sum dpre,  r1 = sum dpre * (z - beta)/gamma,
//   r2 = sum dy * sin(z) (PSine) or sum dy * min(z, 0) (PReLU).  Two-stage column reduction, deterministic (train_decoder.hip).
constexpr int AB_RS = 1024;   // row splits: narrow layers (24-116 channels) have one column block, the splits are what fills the chip (four blocks per CU:
                              // a block keeps only 8 KB of loads in flight, and at one block per CU the pass ran at a quarter of the HBM rate)
struct ActBwdP {
    const float* dy; const float* z; float* dconv;     // [rows][ld]
    int ld_dy, ld_z, ld_dconv;                          // 0 = C
    int64_t rows; int C;
    int act;                                            // ACT_NONE / ACT_SILU / ACT_PSINE / ACT_RELU / ACT_PRELU
    const float* actw;                                  // PSine w / PReLU slope
    const float* scale;                                 // BN scale s (null = 1)
    const float* gamma; const float* beta;              // BN affine (null = no BN)
    float* partials;                                    // [AB_RS][3][C]
    int cs_dy, co_dy, cs_z, co_z;                       // column stride (0 = 1) and offset of dy / z (shuffled channel positions)
};
int act_bwd(const ActBwdP& p, float* d_shift, float* d_gamma, float* d_actw, float* d_convbias, bool accumulate, hipStream_t s, float* totals = nullptr);

// ---- batch-statistics BatchNorm (train mode), train_kernels.hip.  The forward kernels keep their fused "acc*scale + shift" epilogues:
// a STATS PASS of the same kernel first reduces the raw conv output per channel, bn_stats_finalize turns the sums into this batch's
// scale/shift (and updates the running statistics like nn.BatchNorm, momentum 0.1, unbiased running variance), then the real pass runs
// with them.  Backward: act_bwd as for eval statistics (dconv = dpre*scale, totals r0 = sum dpre, r1 = sum dpre*xhat), then
// bn_train_fix subtracts scale*(r0/n + xhat*r1/n).
struct BnLayer {
    const float* gamma; const float* beta; float* rmean; float* rvar; const float* conv_bias;   // canonical tensors (bias may be null)
    float* scale; float* shift;                                                                  // outputs [C] (kept on the tape)
    int C;
};
int bn_stats_finalize(const float* partials, int nblk, int blk_stride, int64_t count, const BnLayer& L, float momentum, hipStream_t s);
int bn_train_fix(float* dconv, int ld_dconv, const float* z, int ld_z, int cs_z, int co_z, const float* gamma, const float* beta, const float* scale,
                 const float* totals, int64_t rows, int C, hipStream_t s);
// depthwise 3x3 stats pass: partials[(rs*2 + k)*C + c], DWS_RS row splits
constexpr int DWS_RS = 1024;
int launch_dwconv_stats(const float* in, int N, int Hi, int Wi, int ldi, int ci_off, int C, int stride, const float* w9, float* partials, hipStream_t s,
                        float* raw_out = nullptr, int ldo = 0, int co_off = 0);     // raw_out: also park the raw conv output (then launch_bn_apply instead of a second conv pass)
int launch_bn_apply(float* x, int64_t rows, int C, int ld, int co_off, const float* scale, const float* shift, hipStream_t s, bool fused = false);

// ---------------------------------------------------------------- encoder kernels (encoder_kernels.hip)
struct FrontendW {          // device pointers into the weight blob
    const float* w;         // [15 slabs (ci*5+kt)][50 (kh*7+kw, padded)][32 (co, padded)]
    const float* scale;     // [24] BN scale
    const float* shift;     // [24]
    const float* slope;     // [24] PReLU
    const float* w3;        // split-bf16 operand planes of w for frontend3d_x3_kernel: [15 slabs][4 steps][3 planes][32 co][16 taps, 48-byte rows];
                            //   channel rows 24-31 are zeros (frontend3d_x3p_kernel takes the zero rows of an absent frame from row 24)
                            //   (null: f32 MFMA kernel)
    int pair = 0;           // with w3: two output frames per block (frontend3d_x3p_kernel) - set by the callers from option "frontend_x3" >= 2
    int solo = 0;           // with pipe: one block per CU (diagnostic option "frontend_solo" with chains overlapping)
    int pipe = 0;           // with pair: the next slab's staging interleaved with the current slab's MFMAs (frontend3d_x3q_kernel) - option "frontend_x3" == 3
    const float* w1;        // the same as ONE plane rounded to nearest even: [15 slabs][4 steps][32 co][16 taps, 48-byte rows] (set by the callers
                            //   of launch_frontend only for a model with "infer_bf16"; takes precedence over w3)
};
// where the clips of a launch live: clip b is clip (b % per) of the (per,3,T,H,W) tensor p[b / per] - the G batches of a grouped pass
// (l2s_inference_multi) stay where their caller put them
constexpr int MAX_GROUP = 8;       // = L2S_MAX_GROUP (include/l2s.h)
struct FrameSrc { const float* p[MAX_GROUP]; int per; };
int launch_frontend(const FrontendW& w, const FrameSrc& video, int B, int T, int H, int W, float* out, hipStream_t s, float* zout = nullptr);
inline int launch_frontend(const FrontendW& w, const float* video, int B, int T, int H, int W, float* out, hipStream_t s, float* zout = nullptr) {
    FrameSrc f{}; f.p[0] = video; f.per = B;
    return launch_frontend(w, f, B, T, H, W, out, s, zout);
}
// ---- ragged groups (l2s_inference_ragged): the clips of up to MAX_GROUP padded batches, each with its own B_g and T_g, as rows of ONE launch chain; the
// encoder works on the real frames only.  Clip c (batch order) owns the compact frames frame0 .. frame0 + len - 1 and the front-end pair blocks
// pair0 .. pair0 + ceil(len / 2) - 1.  The device table is N x RaggedClip (host_table.h).
struct RaggedClip { int g, row, T, len, frame0, pair0; };      // source tensor, row in it, ITS frame pitch T_g, frames of the clip, first compact frame, first pair block
struct RaggedTab { const RaggedClip* clips; const int* pair_clip; int N, Tmax, NF, NP; };      // device table and pair map; clips, row pitch of the decoder, sum len, sum ceil(len / 2)
int64_t ragged_table_words(int N);                                                                                           // masked_kernels.hip
int launch_ragged_table(const RaggedClip* clips_host, int N, RaggedClip* clips_dev, int* pair_clip_dev, hipStream_t s);      // the table, then the pair map
// the ragged form of the default front-end (frontend3d_x3q_kernel): blockIdx.y = pair block; clip c's block j is block (0, 2j) of the clip alone at T = len
// (same slabs, same order: same bits), read in place at pitch T_g, written to compact frames frame0 + 2j (+1).  Frames t >= len are never read.
int launch_frontend_ragged(const FrontendW& w, const FrameSrc& video, const RaggedTab& rg, int H, int W, float* out, hipStream_t s);
// ---- evaluate-shaped ragged groups (l2s_forward_eval_ragged; ragged_eval_kernels.hip): every batch also has its own step count S_g.  The chain decodes all
// N rows for Smax steps at pitch Smax / Tmax; clip c's table entry says which of those rows are its own and where its batch's packed output blocks start.
// Offsets are in floats and fit an int: the largest block set of a call is 256 clips x 300 steps x 300 frames = 23 040 000 floats.
struct EvalClip { int S, T, row, mT, mel_off, stop_off, attn_off, dis_off; };      // S_g, T_g, row in its batch, min_T(T_g), start of ITS BATCH's mel / stop / attention / content_dis block
struct EvalTab { const EvalClip* clips; int N, Smax, Tmax, mTmax; };               // device table; clips, the staging pitches (steps, frames, content slots)
enum EvalField { EV_STOP = 0, EV_ATTN = 1, EV_DIS = 2, EV_MEL_POST = 3 };
int64_t eval_table_words(int N);
int launch_eval_table(const EvalClip* clips_host, int N, EvalClip* clips_dev, hipStream_t s);
int launch_zero_rows_past_s(float* x, int cols, const EvalTab& ev, hipStream_t s);      // x (N * Smax, cols) dense: rows j >= S_c of every clip become zeros
int launch_eval_scatter(int field, const float* src, const EvalTab& ev, float* dst, hipStream_t s);      // a staged output (pitch Smax / Tmax / mTmax) -> the packed blocks
int launch_eval_mel_cf(const float* mel, const EvalTab& ev, float* mel_cf, hipStream_t s);               // mel (N, Smax, 80) row-major -> the packed channel-first blocks
// batch-statistics pass of the front-end conv (training): partials[(block*2 + k)*24 + ch], *nblocks blocks
int launch_frontend_stats(const FrontendW& w, const float* video, int B, int T, int H, int W, float* partials /*[blocks][2][24]*/, int* nblocks, hipStream_t s, float* raw_out = nullptr);
// raw_out (NF,H/2,W/2,24): the statistics pass also parks the raw conv map; launch_bn_apply on it + launch_frontend_pool then replace the second conv pass
int launch_frontend_pool(const float* z, const float* slope, int NF, int Hc, int Wc, float* out, hipStream_t s);

// data boundary: packed uint8 RGB clips (clip i = frames[i] x H x W x 3 bytes at packed + offsets[i]) -> video (B,3,T,H,W) fp32,
// /255 then ImageNet mean/std, clips shorter than T zero-padded; offsets / frames are HOST arrays
constexpr int MAX_COLLATE_CLIPS = 64;        // per launch (the clip table travels in the kernel arguments)
int launch_normalise_pad(const uint8_t* packed, const int64_t* offsets, const int* frames, int B, int T, int H, int W, float* video, hipStream_t s);
// face crops of unequal size (frame_resize.hip): the pure host check of a job table (include/l2s.h's l2s_resize_job), and the check plus the launches
int resize_check(const ::l2s_resize_job* jobs, int n, int64_t packed_bytes, int mode, int B, int T, int oh, int ow);
int launch_resize_normalise(const uint8_t* packed, int64_t packed_bytes, const ::l2s_resize_job* jobs, int n, int mode, int B, int T, int oh, int ow, float* out,
                            hipStream_t s);
// face alignment before those crops (face_align.hip): the pure host check of a job table (include/l2s.h's l2s_align_job), and the check plus the launches
int align_check(const ::l2s_align_job* jobs, int n, int64_t packed_bytes);
int launch_align_faces(const uint8_t* packed_in, int64_t packed_bytes, const ::l2s_align_job* jobs, int n, uint8_t* packed_out, hipStream_t s);
// depthwise 3x3, pad 1, channel-last: in (N,Hi,Wi,ldi) channels [ci_off, ci_off+C) -> out (N,Ho,Wo,ldo) at co_off
int launch_dwconv(const float* in, int N, int Hi, int Wi, int ldi, int ci_off, int C, int stride,
                  const float* w9 /*[9][C]*/, const float* scale, const float* shift,
                  float* out, int ldo, int co_off, hipStream_t s);
// fused stride-1 ShuffleNet unit (encoder_kernels.hip)
struct ShuffleS1P {
    const float* x; float* out;                              // (NF, h, h, 2*half) channel-last
    const float* w1f; const float* s1; const float* b1;      // pw1: frag16 [pad16(half)][Kpad], BN scale/shift
    const float* wd; const float* sd; const float* bd;       // dw: [9][half], BN scale/shift
    const float* w2f; const float* s2; const float* b2;      // pw2
    int NF, h, half, Kpad, F;
    const void* w1p; const void* w2p;                        // pw1 / pw2 as pre-split bf16 operand planes (launch_su_planes) or null: both set -> the split-bf16 unit
};
int64_t su_planes_bytes(int N, int K);
int launch_su_planes(const float* W, int N, int K, void* out, hipStream_t s);      // [N][K] fp32 -> [ceil(N/16)][pad32(K)/32][3 planes][64 lanes] 16 bytes
int launch_shuffle_s1(const ShuffleS1P& p, hipStream_t s);
constexpr int S1_CHAIN_MAX = 7;
int launch_shuffle_s1_chain(const ShuffleS1P* units, int n, hipStream_t s);      // n consecutive stride-1 units of one stage in ONE launch (the map stays on chip between them); same bits
void shuffle_set_timeline(unsigned long long* ts, int h);     // non-null: launch the stamped measurement build (tools/fused_unit_timeline.py)
// fused stride-2 ShuffleNet unit (encoder_kernels.hip): banch1 (dw s2 -> pw) and banch2 (pw -> dw s2 -> pw) of one strip of Ro
// output rows per block; the full-resolution pw1 map (124 MB at B=32 in stage 2) never leaves the CU
struct ShuffleS2P {
    const float* x; float* out;                              // (NF, h, h, cin) -> (NF, ho, ho, 2*half), channel-last
    const float* wd1; const float* sd1; const float* bd1;    // banch1 dw: [9][cin], BN scale/shift
    const float* wb1f; const float* sb1; const float* bb1;   // banch1 pw: frag16 [pad16(half)][Kin]
    const float* w1f; const float* s1; const float* b1;      // banch2 pw1: frag16 [pad16(half)][Kin]
    const float* wd; const float* sd; const float* bd;       // banch2 dw: [9][half]
    const float* w2f; const float* s2; const float* b2;      // banch2 pw2: frag16 [pad16(half)][Kh]
    int NF, h, ho, cin, half, Kin, Kh, Ro;
    const void* wb1p; const void* w1p; const void* w2p;      // the three pointwise weights as pre-split bf16 operand planes (launch_su_planes) or null
};
int launch_shuffle_s2(const ShuffleS2P& p, hipStream_t s);
// out[r*ldo + off_o + c*cs_o] = in[r*ldi + off_i + c]
int launch_copy_cols(const float* in, int ldi, int off_i, float* out, int ldo, int off_o, int cs_o,
                     int64_t rows, int cols, hipStream_t s);
// x (NF, P, C) -> mean over P -> L2 normalise over C -> vis[f*ldv + c]; emb (B,E) tiled into vis[f*ldv + C + e]
int launch_pool_norm_cat(const float* x, int NF, int P, int C, const float* emb, int E, int T,
                         float* vis, int ldv, float* feat /*optional (NF,C)*/, hipStream_t s);
// the ragged form: one block per (clip c, t) of the N x Tmax grid; t < len: compact frame frame0 + t (same sums, same order) + emb[c] -> vis row c*Tmax + t, else a zero row
int launch_pool_norm_cat_ragged(const float* x, const RaggedTab& rg, int P, int C, const float* emb, int E, float* vis, int ldv, hipStream_t s);

// ---------------------------------------------------------------- skinny (batch-row) MFMA kernels (skinny.hip)
// "frag16" layout of a row-major X[R][K] (R padded to 16, K multiple of 16):
//   F[(rt*(K/16) + c)*256 + l*4 + e] = X[16*rt + (l&15)][16*c + 4*(l>>4) + e]      (l = lane 0..63)
// One float4 per lane per 16-deep K chunk = exactly the A (or B) operands of four v_mfma_f32_16x16x4_f32.
__host__ __device__ inline int64_t frag16_index(int row, int k, int K) {
    int rt = row >> 4, i = row & 15, c = k >> 4, g = (k >> 2) & 3, e = k & 3;
    return ((int64_t)(rt * (K >> 4) + c) * 64 + (g * 16 + i)) * 4 + e;
}

enum SkinnyEpi {
    SK_PLAIN = 0,      // out[row*ldo + n] = act(v)                       (+ optional pos/add rows)
    SK_FRAG = 1,       // out frag16 (K = N) = act(v) (+add)
    SK_LSTM = 2,       // LSTM cell: rows of W permuted to (unit, gate); updates h (frag), c (frag)
    SK_MEL = 3,        // fc_out(+stop row): writes mel[b][step][n], y frag16, stop[b][step]
};
struct SkinnySeg { const float* a; int nchunks; };   // one K segment of A in frag16 layout (K = 16*nchunks)
struct SkinnyP {
    SkinnySeg seg[4];
    int nseg;
    const float* a_sum;    // optional second frag16 source of segment 1 (same shape): the segment's operand is seg[1].a + a_sum, added by the loader
                           //   (the decode step's u = prenet + attention_proj(a @ v), decoder.py:421; straight-line four-wave blocks only)
    int layout;            // set by launch_skinny: index of a compile-time segment layout the kernel has an instance for (0 = general path)
    const float* W;        // packed frag16 of the [Npad][K] weight, K = sum of segments
    const void* W3;        // optional: the same weight as three bf16 planes for the split-bf16 LSTM blocks ([tile][K slice 8][chunk pair][plane][lane] 16 B;
                           //   skx_planes_kernel); with it and option "lstm_x3" the launch runs on the bf16 matrix cores
    const float* bias;     // [Npad] (permuted order for SK_LSTM)
    const float* actw;     // [N] psine weights
    const float* add;      // optional plain [B][ld_add] added after activation (SK_PLAIN/SK_FRAG)
    int ld_add;
    const float* addrow;   // optional [N] row added after activation (positional encoding of this step)
    float* out;            // SK_PLAIN: [B][ldo]; SK_FRAG: frag16 with K = N
    int ldo;
    int B, N, K;           // N = valid output columns
    int act;
    int epi;
    // SK_LSTM
    const float* pre;      // optional precomputed input gates: pre[b*ld_pre + gate*H + unit]
    int64_t ld_pre;
    const float* c_in;     // frag16 (K = H) previous cell
    float* c_out;          // frag16
    float* h_out;          // frag16 (K = h_out_K) at column offset h_out_off
    int h_out_K, h_out_off;
    float* h_seq;          // optional plain: h_seq[b*ld_hseq + unit]
    int64_t ld_hseq;
    float* h_plain;        // optional second plain copy
    int ld_hplain;
    int H;
    // SK_MEL
    float* mel; int64_t ld_mel_b;      // mel[b*ld_mel_b + n] (already offset to this step)
    float* stop; int64_t ld_stop_b;    // stop[b*ld_stop_b]   (already offset to this step)
    const float* stop_const;           // [B]
    float* yfrag;                      // frag16, K = 80
    int* es_ctl; int es_end;           // option "early_stop" (else null): the call's EsCtl block; the end step (minus S) to store once the last clip has crossed at this step
    // SK_LSTM on the K = 768 layout of the decode step (option "hoist_vproj" = 3; else null): the content term of the gates, hoisted out of the GEMM
    const float* hoist_p;              // P[b][packed gate row 4 * unit + gate][hoist_pitch] = value_j . W_ih[row, content] (the prologue's table; slots past m_b zero)
    const float* hoist_alpha;          // alpha[b][CONTENT_HOIST_MAX_M]: the step's content soft-max weights, zeros past m_b (the attention launch)
    int hoist_pitch;                   // floats per gate row of P: the clip's content slots rounded up to 4 (4 or 8)
};
// The longest clip (content slots m = T / 7) whose calls take the hoisted content term: a cell thread reads ceil4(m) floats of P per gate and step in place of
// the 256 content columns of the GEMM - 4 m bytes x 2048 gates x rows per launch against 256 columns x 2048 x 6 bytes of weight planes once per 64 rows plus the
// rows' 1 KB of activations.  At m = 4 (T = 29) that is 8.4 MB more and about 5 MB less through the fabric per 256-row launch for a quarter fewer K steps; from
// m = 9 on (three 16-byte requests per gate, 25 MB) the table read outgrows what the columns cost, so longer clips keep the K = 1024 form.
constexpr int CONTENT_HOIST_MAX_M = 8;
inline int content_hoist_pitch(int m) { return m <= CONTENT_HOIST_MAX_M ? (m + 3) / 4 * 4 : 0; }      // 0: no table for this clip length
// Option "early_stop" on the launch-per-phase loop: a per-call control block in the call's own workspace.  The SK_MEL epilogue notes a clip's FIRST stop
// crossing; the one that completes the count lowers the end step (ordinary vector atomics).  Every step kernel carries its step index and returns at its
// top once that index is at or past the end - a uniform branch on a kernel argument that is null when the option is off.  Steps are kept RELATIVE to S
// (end_rel = end - S <= 0, es_step = step - S < 0), so that one memset to zero arms the block: "run to S".
struct EsCtl { int end_rel; int count; int crossed[1]; };      // crossed[B]
constexpr int ES_POST_LAYERS = 5, ES_POST_TAPS = 5;
constexpr int ES_MARGIN = ES_POST_LAYERS * (ES_POST_TAPS / 2);      // post-net frame j reads pre-post-net frames j - 10 .. j + 10 (five Conv1d layers, kernel 5, pad 2);
                                                                    //   19 where layers 1-3 run in Winograd form (l2s_api.hip ES_MARGIN_WINO)
constexpr int SKINNY_MAX_GROUP = 4;
struct SkinnyBatch { SkinnyP p[SKINNY_MAX_GROUP]; int ntiles[SKINNY_MAX_GROUP]; int count; const int* es_end; int es_step; };
#define L2S_ES_RETURN(arg) do { if ((arg).es_end && (arg).es_step >= *(arg).es_end) return; } while (0)
int launch_skinny(const SkinnyBatch& b, hipStream_t s, const char* name, const Options& o = Options());
int launch_skx_planes(const float* Wf, int ntiles, int K, void* out, hipStream_t s);      // bf16 planes of a packed LSTM weight (SkinnyP::W3): ntiles * K * 16 * 6 bytes
bool skinny_sum_supported(const Options& o);           // does LSTM layer 0's launch with SkinnyP::a_sum have a block form under these options (skinny.hip skinny_form, step 5)?
void attn_set_timeline(unsigned long long* ts);        // non-null: the stamped attention kernel (tools/attn_timeline.py)
void skinny_set_flat_timeline(unsigned long long* ts);   // non-null: the stamped build of the step's flat first phase (tools/flat_timeline.py)
void skinny_set_timeline(unsigned long long* ts);      // non-null: launch the stamped measurement build (tools/skinny_timeline.py)

int launch_probe(int kind, int blocks, int n_per_block, const float* in, float* out, hipStream_t s);      // libl2s_diag.so only, like every *_set_timeline above
void skinny_set_flat_timeline(unsigned long long* ts);
int set_stamp_log(unsigned long long* log, long long cap);      // the block-stamp log of the step kernels (skinny.hip; libl2s_diag.so only)
// the kernel launch_skinny would launch for this (validated) batch - the ES = false entry of the dispatcher's row - with its launch shape; null, and the
// error set as launch_skinny sets it, where it would refuse.  Launches nothing (skinny.hip; libl2s_diag.so only)
const void* skinny_form_kernel(const SkinnyBatch& bl, const Options& o, int chains, bool stamped_skinny, bool stamped_flat, dim3& grid, int& block, int& lds);

// ---------------------------------------------------------------- decoder helper kernels (decoder_kernels.hip)
struct AttnP {
    const float* q; int ldq;          // [B][512]
    const float* k;                   // [B][T][512]
    const float* v;                   // [B][T][512]
    const float* vp;                  // optional [B][T][256] = V W_ap^T + b_ap: then av_frag receives o = a @ V' (frag16, K = 256) instead of a @ v
    const float* tau;                 // device scalar
    float* av_frag;                   // frag16, K = 512
    float* attn_out; int64_t ld_attn_b; int attn_logits;   // optional [b*ld + t]
    const float* qc; int ldqc;        // [B][256]
    const float* ckey;                // [B][m][256]
    const float* cval;                // [B][m][256]
    const float* tau_c;
    float* cc_frag;                   // frag16, K = 256
    float* alpha_out;                 // option "hoist_vproj" = 3 (else null): alpha[b][CONTENT_HOIST_MAX_M] is stored, zeros past the clip's slots, INSTEAD of cc = alpha @ value
    int B, T, m;
    const int* es_end; int es_step;   // option "early_stop" (else null): the launch returns at once when es_step (step - S) >= *es_end (EsCtl::end_rel)
};
// attention role + second prenet layer in one grid (skinny.hip)
int launch_step_attn(const AttnP& at, const SkinnyP& pre2, int pre2_tiles, hipStream_t s, int lds_values = 1, int skip0 = 0);
// adaptive average pooling of up to 5 channel-last maps into a concatenated (B, m, nmaps*C) buffer
struct PoolCatP { const float* x[5]; int L[5]; int ld[5]; int nmaps; int B, m, C; float* out; };
int launch_pool_cat(const PoolCatP& p, hipStream_t s);
// rows softmax: z = softmax((l+g)/tau) into zpad [rows][ldz] (zero padded), dis = softmax(l) (optional)
int launch_gumbel_softmax(const float* logits, const float* gumbel, int rows, int n, float tau,
                          float* z, int ldz, float* dis, hipStream_t s);
// plain [B][K] -> frag16 (rows padded with zeros); K multiple of 16; optional broadcast of a single row
int launch_to_frag(const float* x, int ldx, int B, int K, float* frag, int Kfrag, int koff, int broadcast_row, hipStream_t s);
int launch_fill(float* p, int64_t n, float v, hipStream_t s);
// frag16 -> plain: out[b*ldo + ooff + k] = frag[b][k]
int launch_from_frag(const float* frag, int Kfrag, int B, int K, float* out, int ldo, int ooff, hipStream_t s);
// dst[(b*T + t)*ldd + c] = src[b*lds + c]
int launch_tile_rows(const float* src, int lds, float* dst, int ldd, int B, int T, int C, hipStream_t s);
// (B,S,C) -> (B,C,S)
int launch_transpose_bsc(const float* in, int B, int S, int C, float* out, hipStream_t s);
int launch_output_lengths(const float* stop, int B, int S, int64_t* lengths, hipStream_t s);
// option "early_stop": mel_post[b][:][j] = 0 and attn[b][j][:] = 0 (attn may be null) for j >= lengths[b]
int launch_mask_by_lengths(const int64_t* lengths, int B, int S, int T, float* mel_post, float* attn, hipStream_t s);
// ---- per-clip video lengths (masked_kernels.hip; the *_masked entry points).  The device length table is 2*B int32: len_b, then m_b = l2s_min_T(len_b)
int64_t len_table_words(int B);
int launch_len_table(const int32_t* lens_host, int B, int* table, hipStream_t s);
// forward BiLSTM rows with len_b - 1 == t: h (frag16) -> h_dst_frag (same row), c (frag16) -> c_dst[b*ld_c + unit]
int launch_bilstm_capture(const float* h_frag, const float* c_frag, const int* lens, int B, int t, float* h_dst_frag, float* c_dst, int ld_c, hipStream_t s);
// backward BiLSTM rows with len_b - 1 == t: h = c = s_e[b] (frag16 buffers)
int launch_bilstm_reset(float* h_frag, float* c_frag, const int* lens, int B, int t, const float* s_e, hipStream_t s);
// x rows (b, t >= len_b) := 0 in place; out := x (the masked copy)
int launch_mask_copy_rows(float* x, int ldx, float* out, int ldo, const int* lens, int B, int T, int cols, hipStream_t s);
struct PoolDiv { int div[5]; };                                // map j of a clip of len frames has len / div[j] valid positions
int launch_pool_cat_masked(const PoolCatP& p, const PoolDiv& d, const int* lens, hipStream_t s);
int launch_zero_slot_rows(float* z, int ldz, float* dis, int n, int B, int m, const int* lens, hipStream_t s);
// launch_step_attn with per-row lengths: row b's soft-max and a @ V' over t < len_b (attention columns past it: 0, or -inf for logits), content over m_b slots
int launch_step_attn_masked(const AttnP& at, const SkinnyP& pre2, int pre2_tiles, const int* lens, hipStream_t s, int lds_values = 1, int skip0 = 0);
// ---- per-clip video lengths on the training path (masked_train.hip; the l2s_train_*_masked_fwd / _masked_bwd entry points).  The device table is 3*B int32: the two
// segments above, then frame0_b = sum of len_c over c < b (clip b's first frame in the encoder trunk's compact frame list)
int check_lengths(const int32_t* video_lengths, int B, int T);      // l2s_api.hip: every len_b in [7, T], else an error that names the row
int64_t train_len_table_words(int B);
int launch_train_len_table(const int32_t* lens_host, int B, int* table, hipStream_t s);
// rows of `cols` floats between the padded layout (row b*T + t) and the compact one (row frame0_b + t): to_compact gathers the real rows; otherwise the
// padded rows are written from the compact ones, rows t >= len_b as zeros
int launch_frame_rows(const float* src, float* dst, const int* lens, int B, int T, int64_t cols, bool to_compact, hipStream_t s);
// compact normalised features (sum len, C) -> vis rows [feat | emb_b] and / or feat rows of the padded batch; feature columns of rows t >= len_b are zeros
int launch_feat_rows_store(const float* featc, int C, const float* emb, int E, const int* lens, int B, int T, float* vis, int ldv, float* feat, hipStream_t s);
// dfeat rows (stride ld_df) of the real frames -> compact (sum len, C); rows t >= len_b are never read
int launch_feat_rows_gather(const float* dfeat, int ld_df, int C, const int* lens, int B, int T, float* out, hipStream_t s);
// launch_bilstm_reset that also writes the post-reset state into the tape's predecessor rows (plain (B,512) each)
int launch_bilstm_reset_tape(float* h_frag, float* c_frag, float* hprev, float* cprev, const int* lens, int B, int t, const float* s_e, hipStream_t s);
// adjoint of the capture: dh_last (B,512) = dh_init where len_b == T, else 0 with dc_carry[b] = 0 and drnn[b][len_b - 1][0:512] += dh_init[b] ...
int launch_bilstm_capture_adj_init(const float* dh_init, float* dh_last, float* dc_carry, float* drnn, int ld_rnn, const int* lens, int B, int T, hipStream_t s);
// ... and dc_carry[b] = dcell[b] for the rows with len_b == len
int launch_bilstm_capture_adj_cell(const float* dcell, int ld_dcell, float* dc_carry, const int* lens, int B, int len, hipStream_t s);
// adjoint of the reset, rows with len_b == len: gate gradients (frag16, K = 2048) move to dg_reset, the carried cell gradient to ds_e; both are cut
int launch_bilstm_reset_adj(float* dg_frag, float* dg_reset, float* dc_carry, float* ds_e, const int* lens, int B, int len, hipStream_t s);
// rows t >= lens[b] of x (B*T rows, ldx) := 0 over `cols` columns (lens: segment 0 of a video-length or a mel-length table; `name`: the profile scope)
int launch_zero_pad_rows(float* x, int ldx, const int* lens, int B, int T, int cols, hipStream_t s, const char* name = "train_bwd_zero_pad_rows");
// ---- per-clip mel lengths on the training path (masked_mel.hip; l2s_loss_lengths and the l2s_train_postnet_masked_fwd / _masked_bwd entry points).  The device
// table is 2*B int32: S_b, then m_b = the clip's content rows (video_lengths[b] / 7; m without video lengths).  Segment 0 is what launch_zero_pad_rows reads
int check_mel_lengths(const int32_t* mel_lengths, int B, int S);      // B in [1, 96] and every S_b in [1, S], else an error that names the clip
int64_t mel_len_table_words(int B);
int launch_mel_len_table(const int32_t* mel_lengths, const int32_t* video_lengths, int B, int m, int* table, hipStream_t s);
int launch_zero_cf_past_len(float* x, const int* lens, int B, int C, int S, hipStream_t s);      // x (B, C, S) channel-first: positions s >= S_b := 0
// the 4-term loss of train_kernels.hip (l2s_loss): term 0 = sum (a-b)^2 over mel, 1 = same for mel_post, 2 = BCE sum, 3 = KLD sum; gradients in the same pass
struct LossP {
    const float* mel; const float* mel_post; const float* mel_tgt;    // (B,80,S) channel-first, like the reference's outputs
    const float* stop; const float* gate;                            // (B,S)
    const float* dis;                                                // (R,V)
    float* dmel; float* dmel_post; float* dstop; float* ddis;        // gradients of the summed loss (may be null)
    int64_t n_mel, n_stop, n_dis; int R, V;
};
int launch_loss(const LossP& p, double* partials /*[4*1024]*/, float* out5, hipStream_t s);
// backward of the adaptive average pooling + concatenation: dp (B,m,nmaps*C) -> d map_j; acc[j]: add to dx[j].  The masked form matches pool_cat_masked's bins
struct PoolCatBwdP { float* dx[5]; int L[5]; int ld[5]; int acc[5]; int nmaps; int B, m, C; const float* dp; };
int launch_pool_cat_masked_bwd(const PoolCatBwdP& p, const PoolDiv& d, const int* lens, hipStream_t s);
int launch_frame_window(const float* audio, int B, int N, int L, int n_fft, int hop, const float* window, float* frames, hipStream_t s);
int launch_power(const float* spec, int lds, int64_t rows, int nf, float* power, int ldp, hipStream_t s);
// ---- the voice tower over clips of unequal length (l2s_speaker_encoder_packed): the time-major compact layout - frame l of the clip of rank r (clips
// by frame count descending) is row step_row0[l] + r.  Device table (host_table.h): B x SpkRank, then step_row0[0 .. L_max]
struct SpkRank { int64_t off; int32_t n; int32_t b; };         // the clip of one rank: float offset into the packed audio, samples, index in call order
int launch_frame_window_packed(const float* audio_packed, const SpkRank* ranks, const int* step_row0, int B, int L_max, int n_fft, int hop, const float* window,
                               float* frames, hipStream_t s);
// h_last[b] = hseq[step_row0[L_b - 1] + rank(b)], 256 wide, in call order
int launch_spk_last_hidden(const float* hseq, const SpkRank* ranks, const int* step_row0, int B, float* h_last, hipStream_t s);
// ---------------------------------------------------------------- mel filterbank band tables (vocoder.hip; read by l2s_inverse_mel and l2s_mel_targets)
constexpr int IM_MAXF = 576;      // 9 bins per lane
constexpr int IM_MAXM = 128;      // 2 mel bands per lane
constexpr int IM_NNZ = 2048;      // capacity of each compact table (the 513 x 80 HTK filterbank has ~1 100 non-zeros)
// fb dev (n_freqs, n_mels) -> tab: [n_mels][3] first bin / last+1 / offset into fwd; [n_freqs][3] first band / last+1 / offset into bwd; then the two totals
// (3 (n_mels + n_freqs) + 2 ints); fwd / bwd (IM_NNZ floats each): fb's values over those ranges, band-major / bin-major.  One block, on `s`
int launch_mel_bands(const float* fb, int n_freqs, int n_mels, int* tab, float* fwd, float* bwd, hipStream_t s);
// stop_const[b] = dot(ecell[b], w[512:1024]) + bias
int launch_stop_const(const float* ecell, const float* w_tail, const float* bias, int B, float* out, hipStream_t s);

}  // namespace l2s
