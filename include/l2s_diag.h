/*
 * l2s_diag.h - the DIAGNOSTIC surface of the MI355X-native Lip2Speech hot path (libl2s_diag.so).
 *
 * libl2s_diag.so is built from the sources of libl2s_hip.so with -DL2S_DIAG (lip2speech_amd/csrc/Makefile).  It exports the whole product
 * ABI of l2s.h (same kernels, same launch code) PLUS what only measurements and operator tests need:
 *   - operator-level entry points (one GEMM / Conv1d / front-end conv) for the operator parity tests,
 *   - chain microbenches and launch-floor probes,
 *   - stamped ("timeline") builds of the kernels and the block-stamp log behind the overlap proof of profiles/,
 *   - the run-time switches that only choose between block forms of the same arithmetic (measured-and-rejected forms kept for A/B timing),
 *   - the test hook of the persistent loop's give-up path (environment variable L2S_TEST_PDECODE_STARVE).
 * None of this is in libl2s_hip.so, and the package (lip2speech_amd/native.py lib(), the callers, bench.py's timed region) never loads this
 * library: tools/ set L2S_LIB to it, tests bind it through native.diag().  An l2s_model created by one library may be handed to the other
 * (same struct, same process heap, same device context).
 */
#ifndef L2S_DIAG_H
#define L2S_DIAG_H

#include "l2s.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- diagnostic run-time options (l2s_set_option / l2s_model_set_option of libl2s_diag.so accept these on top of l2s.h's; the product library
 * answers "unknown option").  Defaults are the forms the product runs; every other value selects a form that measured slower or equal:
 *   "fuse_trunk"        (1)  stride-1 ShuffleNet units as one fused kernel each; 0 = pw/dw/pw/copy launches
 *   "fuse_s2"           (1)  stride-2 ShuffleNet units as one fused kernel each (needs fuse_trunk); 0 = dw/pw + pw/dw/pw launches
 *   "overlap_postnet"   (0)  l2s_inference: windowed post-net on a second stream under the decode loop
 *   "gemm_x3_dma"       (1)  constant weights of the split-bf16 GEMMs as pre-split bf16 planes by LDS-DMA; 0 = load + split + LDS store in the staging waves
 *   "hoist_vproj"       (3)  attention_proj applied to the VALUES once per clip in the prologue: 3 = also the content columns of LSTM0 applied to the content
 *                            values once per clip: LSTM0 on [prenet + o | h0] (K = 768), the content term added by the cell threads from the state's
 *                            L2S_ST_CP table (clips of at most 8 content slots; longer clips run 2), 2 = LSTM0 on [content | prenet + o | h0] (K = 1024), 1 = on
 *                            [content | prenet | o | h0] (K = 1280), 0 = a @ v through the pre-multiplied W_ih W_ap (K = 1536)
 *   "attn_lds"          (1)  attention blocks with the projected values staged through LDS: 1 = at up to 128 rows and whenever chains overlap, 2 = always, 0 = never
 *   "flat_half"         (1)  the step's first launch on four-wave half-CU blocks when chains overlap; 2 = always, 0 = never
 *   "half_min_mts"      (12) with "lstm_x3" >= 3 and chains overlapping: an all-LSTM launch takes the half-CU 4x2 / shared-panel form from this many 16-row tiles on
 *   "trunk_chain"       (1)  the stride-1 units of ShuffleNet stages 2 and 3 as ONE launch per stage (the map stays on chip between the units); 2 = stage 4 too, 0 = one launch per unit
 *   "post_wino"         (1)  post-net layers 1-3 (Conv1d 512 -> 512, 5 taps) in their Winograd F(4,5) form - input transform, eight K = 512 products in one grouped
 *                            split-bf16 launch, output transform - on the plain full-range route: 1 = from 4 096 rows per batch on, 2 = at any row count, 0 = never
 *   "frontend_solo"     (0)  when chains overlap, the front-end conv one block per CU (an LDS pad) so that other chains' step kernels run beside it: measured -8 %, off
 *   "flat_xcd"          (1)  the step's first launch with an XCD-affine block -> tile map (an XCD = one row half x one column quarter of a group); 0 = row-major
 *   "attn_skip0"        (1)  when chains overlap, attention blocks fetch only the projected-value rows whose soft-max weight is not exactly zero; 2 = always, 0 = never
 *   "skinny_flat"       (1)  multi-group batch-row launches at >= 128 rows as one flat grid of per-group block shapes; 0 = one shape for all groups
 *   "skinny_rc"         (0)  batch-row kernels at >= 64 rows: 0 = by tile count, 11 = 1x1 blocks only, 21 / 22 / 42 = force RT x CT tiles;
 *   "skinny_rc_multi"   (0)  the same for launches that carry several GEMM groups;  "skinny_rc_jb" (0): operand batching of those blocks (2 / 4 / 15 / 28 / 44)
 *   "skinny_static"     (0)  compile-time K-segment layouts in the 16x16 batch-row kernels;  "skinny_sized" (1): instances sized for the launch's longest K;
 *   "skinny_split"      (2) / "skinny_split8" (1): operand loads of the K <= 1536 / K <= 1024 instance in this many batches */

/* ---- operator-level entry points (the operator parity tests of tests/test_gpu_parity.py) -------- */
/* C[M,N] = act((A[M,K] @ Wt[N,K]^T) * scale[N] + shift[N]);  act: 0 none, 1 relu, 2 silu, 3 sin(x)*actw[n] */
int l2s_op_gemm(const float* A, const float* Wt, const float* scale, const float* shift, const float* actw,
                float* C, int M, int N, int K, int act, void* stream);
/* Conv1d over channel-last sequences as an implicit GEMM: X (B,Tin,Cin), Wp (Cout, taps*Cin) with
 * k = tap*Cin + ci, out (B,Tout,Cout), Tout = (Tin + 2*pad - taps)/stride + 1 */
int l2s_op_conv1d(const float* X, const float* Wp, const float* scale, const float* shift, const float* actw,
                  float* out, int B, int Tin, int Cin, int Cout, int taps, int stride, int pad, int act,
                  void* stream);
/* the same two operators with flags: bit 0 = run on the split-bf16 kernel (fp32 operands split into 3 bf16 planes, six bf16 MFMAs per
 * K step; eligible shapes only - otherwise the f32 kernel runs); bit 1 = bf16 operands (round to nearest even on the way into LDS, one
 * bf16 MFMA per K step, fp32 accumulation); bit 2 (with bit 0) = the split-bf16 kernel's 128x128x32 tile instead of its default 128x256x32 one
 * (same bits out; kept for A/B timing); bit 3 (with bit 0) = the weight operand as pre-split bf16 planes fetched by LDS-DMA - what a model with
 * "gemm_x3_dma" runs in its post-net - derived per call into scratch memory the library owns (N % 256 == 0, K % 16 == 0, else ignored; same bits out) */
int l2s_op_gemm_ex(const float* A, const float* Wt, const float* scale, const float* shift, const float* actw, float* C, int M, int N,
                   int K, int act, int flags, void* stream);
int l2s_op_conv1d_ex(const float* X, const float* Wp, const float* scale, const float* shift, const float* actw, float* out, int B,
                     int Tin, int Cin, int Cout, int taps, int stride, int pad, int act, int flags, void* stream);
/* backward of l2s_op_conv1d (no scale/shift/activation): dZ (B,Tout,Cout), X (B,Tin,Cin), Wp (Cout, taps*Cin) ->
 * dX (B,Tin,Cin) (stride 1 only; may be NULL) and dWp (Cout, taps*Cin) (may be NULL) */
int l2s_op_conv1d_bwd(const float* dZ, const float* X, const float* Wp, float* dX, float* dWp, int B, int Tin, int Cin, int Cout, int taps,
                      int stride, int pad, void* stream);
/* fused Conv3d(3->24,5x7x7,s(1,2,2),p(2,3,3)) + BN + PReLU + MaxPool(1,3,3)/s(1,2,2)/p(0,1,1) of the model:
 * video dev (B,3,T,H,W) -> out dev (B*T, H/4, W/4, 24) channel-last */
int l2s_op_frontend(l2s_model* m, const float* video, int B, int T, int H, int W, float* out, void* stream);
/* one Conv2d of the face tower's implicit-GEMM kernel (face_tower.hip, split-K by the same per-image rule as the tower):
 * x dev NHWC (B,H,W,Cin) when x_bstride == 0, else the NCHW view image b at x + b*x_bstride, (Cin,H,W) contiguous; w dev [Cout][kh][kw][Cin];
 * y dev NHWC (B,Ho,Wo,Cout) = act((conv * scale[n] + shift[n]) + res), res NHWC like y or NULL, act = ReLU if relu */
int l2s_op_face_conv2d(const float* x, int64_t x_bstride, int B, int H, int W, int Cin, const float* w, const float* scale, const float* shift,
                       const float* res, int relu, float* y, int Cout, int kh, int kw, int stride, int ph, int pw, void* stream);
/* l2s_face_encoder_fwd plus stage taps: taps = 8 dev pointers (each may be NULL) receiving, channel-last, conv2d_4b and repeat_1 (B,17,17,256),
 * mixed_6a and repeat_2 (B,8,8,896), mixed_7a and block8 (B,3,3,1792), the pooled features (B,1792) and last_bn's output (B,512) */
int l2s_op_face_taps(l2s_model* m, const float* faces, int64_t batch_stride, int B, float* const* taps, float* proj, float* emb, void* ws,
                     int64_t ws_bytes, void* stream);
/* l2s_speaker_encoder_fwd plus stage taps: taps = 7 dev pointers (each may be NULL) receiving, with R = B * L rows (L = n_samples / 160 + 1 frames per
 * clip), the DFT product spec (R,402) = [re | im], the power spectrum (R,204; columns 201-203 zero), the mel (R,40), the hidden sequences of the three
 * LSTM layers (B,L,256) each, and the Linear + ReLU output (B,256) before normalisation.  Same kernels, same launches: each tap is a device-to-device
 * copy put on the stream after its stage (layer 0's sequence shares its workspace buffer with layer 2's) */
int l2s_op_speaker_taps(l2s_model* m, const float* audio, int B, int n_samples, float* const* taps, float* emb, void* ws, int64_t ws_bytes, void* stream);
/* l2s_speaker_encoder_packed plus the same seven taps in ITS row layout (l2s_speaker_packed_plan: frame l of the clip of rank r is row
 * step_row0[l] + r of R): spec (R,402), power (R,204), mel (R,40), the three hidden sequences (R,256) each, and the Linear + ReLU output (B,256)
 * in call order.  One body with the product entry point, as above */
int l2s_op_speaker_taps_packed(l2s_model* m, const float* audio_packed, const int64_t* offsets, const int64_t* n_samples, int B, float* const* taps, float* emb,
                               void* ws, int64_t ws_bytes, void* stream);
/* l2s_encoder_fwd plus stage taps: taps = 18 dev pointers (each may be NULL) receiving, with NF = B * T frames, channels last: [0] the front-end map
 * (NF, H/4, H/4, 24); [1 + u] the output of ShuffleNet unit u = 0 .. 15 in its shuffled channel order, (NF, h, h, cout) with h = H/8 and cout = 116 for
 * u = 0 - 3, ceil(H/16) and 232 for u = 4 - 11, ceil(H/32) and 464 for u = 12 - 15 - what the trunk's ping-pong buffers hold; [17] the conv_last output
 * (NF * h * h, 768) before pooling.  Same kernels, same launches: each tap is a device-to-device copy put on the stream after the launch that wrote the
 * buffer.  A unit interior to a stage-chain launch (option "trunk_chain": by default units 1 - 2 and 5 - 10, at 2 also 13 - 14) never reaches memory:
 * a non-NULL pointer for it fails the call before anything is launched, with a message that names the unit.  ws_bytes >= l2s_workspace_bytes(B,T,H,W,1),
 * else the call fails before it launches anything.  The padded call only (no ragged groups) */
int l2s_op_encoder_taps(l2s_model* m, const float* video, int B, int T, int H, int W, float* const* taps, float* feat, void* ws, int64_t ws_bytes,
                        void* stream);
/* average duration (us) of the decoder LSTM-cell kernel over a chain of n_pairs x {layer 0, layer 1} launches bracketed by ONE pair
 * of HIP events on `stream` (bench.py's roofline figure; synchronises) */
int l2s_op_lstm_cell_chain(l2s_model* m, int B, int n_pairs, void* ws, int64_t ws_bytes, void* stream, double* avg_us);
/* launch-floor probe: n dependent launches of an empty kernel (kind 0) or of a kernel in which each of `blocks` 512-thread
 * blocks streams n_per_block x 8 KiB from `in` (kind 1) - the cost model of a latency-bound decode phase (tools/launch_floor.py) */
int l2s_op_launch_chain(int kind, int n_launches, int blocks, int n_per_block, const float* in, float* out, void* stream);
/* measurement: with ts_dev != NULL every batch-row ("skinny") launch runs a stamped build of the same kernel - thread 0 of each block
 * writes 8 x 64-bit 100 MHz wall-clock stamps (entry, parameters in SGPRs, loads issued, first operands landed, MFMAs done, after the
 * reduction barrier, after the gate barrier, stores drained) to ts_dev[block*8 ..]; NULL restores the production kernel */
int l2s_op_skinny_timeline(void* ts_dev);
/* the same for the attention blocks of the step's second launch: 8 x uint64 per block (entry, requests issued, q visible, logits, after the barrier,
   weights visible, stored) of the 100 MHz wall clock.  tools/attn_timeline.py */
int l2s_op_attn_timeline(void* ts_dev);
/* and for the step's first launch (the flat grid of per-group block shapes, at >= 128 rows): 8 stamps per block as for l2s_op_skinny_timeline; the last
   such launch leaves its stamps.  tools/flat_timeline.py */
int l2s_op_flat_timeline(void* ts_dev);
/* persistent decode loop (option "persist_decode"): ts_dev = [256 workgroups][16] uint64 stamps of step `step` (100 MHz clock), or NULL to stop */
int l2s_op_pdecode_timeline(void* ts_dev, int step);
/* measurement build of the split-bf16 GEMM: lane 0 of each of the eight waves of block `block` stamps the shader clock per K tile
   ([12 waves][96 K tiles][8 slots] uint64); NULL switches it off again.  tools/gemm_x3_timeline.py */
int l2s_op_gemm_x3_timeline(void* ts_dev, int block);
/* measurement: the same for the fused stride-1 ShuffleNet units of spatial size h (12, 6 or 3; the last such launch leaves its stamps) - 10 x 64-bit words per block to ts_dev[block*10 ..]: 8 stamps (entry,
 * input in LDS, after the barrier, pw1 done, depthwise taps done, depthwise written, pw2 done, stores drained), HW_ID, XCC_ID.  h = -24 / -12 / -6: the
 * stride-2 unit whose INPUT map is that size (9 stamps: entry, input issued, after the barrier, banch1 depthwise, banch2 pw1, banch2 depthwise, banch1 pw,
 * banch2 pw2, stores drained; block = frame * strips + strip).  ([wave][96 K tiles][8 slots] for the GEMM hook above.) */
int l2s_op_fused_unit_timeline(void* ts_dev, int h);
/* measurement: n back-to-back launches of the decode step's attention kernel alone on the state of l2s_decoder_prologue (zero queries): whether a
 * clip's K / V survive in its XCD's L2 between launches when nothing else runs in between (tools/attn_l2_probe.py; workspace: l2s_workspace_bytes) */
int l2s_op_step_attn_chain(l2s_model* m, float* state, int B, int T, int n_launches, void* ws, int64_t ws_bytes, void* stream);
/* the same chain issued alternately on two streams (two independent dependency chains): does a second chain hide the launch floor? */
int l2s_op_launch_chain2(int kind, int n_launches, int blocks, int n_per_block, const float* in, float* out, void* stream_a, void* stream_b);
/* Block-stamp log (the overlap proof of profiles/rNN_overlap_stamps.txt): with log_dev != NULL every block of the decode step's kernels - LSTM launches,
 * first phase, attention - appends one record {entry stamp, exit stamp, tag} of 3 x uint64 (100 MHz constant clock, s_memrealtime; tag = kernel kind
 * 1 LSTM / 2 first phase / 3 attention in bits 60-63, the low 48 bits of a per-chain operand pointer below) to log_dev[1 + 3 * slot ..], slot taken
 * from the atomic counter at log_dev[0]; capacity in records; records past it are dropped (the counter keeps counting).  NULL switches it off. */
int l2s_op_stamp_log(void* log_dev, int64_t capacity);

/* Which kernel would launch_skinny (every launch of the decode step, of the BiLSTM recurrence and of the speaker LSTMs) pick?  The batch is described by
 * integers: `groups` = count x 8 ints {chunks of 16 columns in each of the four K segments, output tiles, epilogue (0 plain, 1 frag16, 2 LSTM cell, 3 mel +
 * stop), weight planes present, summed segment present}, B rows.  The options are those of model m (l2s_model_set_option; it need not be finalised);
 * chains = launch chains in flight (l2s_set_thread_chains), stamped_* = the stamped build of l2s_op_skinny_timeline / l2s_op_flat_timeline armed.
 * Writes one line into out[cap]: the kernel with its template arguments (without the early-stop flag), "grid=(x,y,z) block=N lds=BYTES" - or "ERROR "
 * and the error text where the launch would be refused.  Launches nothing and needs no device. */
int l2s_op_skinny_form(l2s_model* m, int count, const int* groups, int B, int chains, int stamped_skinny, int stamped_flat, char* out, int cap);

/* What the library launches at a call site of launch_skinny, in the integers of l2s_op_skinny_form: the step builders of csrc/decode_step.h - the ones
 * the decode loop, the training forward, the prologue and the voice tower call - run for B rows on dummy operands, under the options of the finalised
 * model m with the ones the site stands for laid over them ("fold_step_weights", "hoist_vproj").  site: a key of "sites" in
 * tests/golden/skinny_forms.json (bilstm_step, phase_a_unfolded, phase_a_folded_step0, phase_a_folded, step_attention_proj, phase_d_k1536,
 * phase_d_k1280, phase_d_k1024_sum, phase_d_k1024_unfolded, phase_e, step_fc_out_stop, spk_lstm_step) or phase_d_k768_hoist ("hoist_vproj" = 3, the
 * integers of tests/test_content_hoist_gpu.py).  Writes *count groups (at most 4) of 8 ints
 * into groups[32].  Launches nothing (tests/test_step_sites_gpu.py). */
int l2s_op_step_site(l2s_model* m, const char* site, int B, int* groups, int* count);

/* One batch-row launch on its own: the operator-level entry of launch_skinny (tests/test_skinny_op_gpu.py; lip2speech_amd/native.py op_skinny packs plain
 * tensors into these layouts).  A group is described as for l2s_op_skinny_form - nchunks[4], ntiles, epi; "W3 set" = planes != NULL, "a_sum set" =
 * a_sum != NULL - plus what the launch reads and writes, all device pointers, with the meaning of the SkinnyP field of the same name (l2s_common.h):
 *   seg_a[j]   frag16 [pad16(B)][16 * nchunks[j]] activations of K segment j (ignored where nchunks[j] == 0); a_sum like seg_a[1] or NULL
 *   W          frag16 [16 * ntiles][K] weight, K = 16 * sum(nchunks); bias [16 * ntiles] or NULL (SK_LSTM: both in the packed row order 4 * unit + gate)
 *   planes     NULL, or a buffer of ntiles * K * 16 * 6 bytes: the call derives the bf16 planes of W into it (launch_skx_planes, K % 256 == 0) on `stream`
 *              and hands them to the launch as SkinnyP::W3
 *   actw [N], add plain [B][ld_add], addrow [N] (each may be NULL); out plain [B][ldo] (SK_PLAIN) or frag16 with K = ldo (SK_FRAG)
 *   SK_LSTM:   pre plain [B][ld_pre] in gate-major order gate * H + unit (or NULL), c_in / c_out frag16 (K = H), h_out frag16 (K = h_out_K) at column
 *              h_out_off, h_seq plain [B][ld_hseq] and h_plain plain [B][ld_hplain] (each may be NULL)
 *   SK_MEL:    mel plain [B][ld_mel_b], stop plain [B][ld_stop_b], stop_const [B], yfrag frag16 (K = 80) or NULL
 * The struct holds its pointers first, then the 64-bit and the 32-bit integers, so that it has no padding. */
typedef struct l2s_skinny_group {
    const float* seg_a[4]; const float* a_sum; const float* W; void* planes; const float* bias; const float* actw; const float* add; const float* addrow;
    float* out; const float* pre; const float* c_in; float* c_out; float* h_out; float* h_seq; float* h_plain;
    float* mel; float* stop; const float* stop_const; float* yfrag;
    int64_t ld_pre, ld_hseq, ld_mel_b, ld_stop_b;
    int32_t nchunks[4], ntiles, epi, N, act, ldo, ld_add, H, h_out_K, h_out_off, ld_hplain;
} l2s_skinny_group;
/* B rows, `count` groups (1 - 4), the options of model m (it need not be finalised), the launch chains of l2s_set_thread_chains.  es_end != NULL: the
 * early-stop twin of the kernel, which returns at its top when es_step >= *es_end (a device int); the stop bookkeeping (SkinnyP::es_ctl) stays off.
 * The batch goes through launch_skinny - its validation, the form rule and the dispatch table of every product launch.  A refused launch returns
 * non-zero with the text in l2s_last_error (the text l2s_op_skinny_form answers after "ERROR "). */
int l2s_op_skinny(l2s_model* m, int count, const l2s_skinny_group* groups, int B, const int* es_end, int es_step, void* stream);
/* The same for ONE SK_LSTM group on the K = 768 layout of the decode step (nchunks = {0, 16, 32, 0} with a_sum: option "hoist_vproj" = 3) with the hoisted
 * content term: hoist_p [B][16 * ntiles][hoist_pitch] (rows in the packed order 4 * unit + gate), hoist_alpha [B][8] (zeros past the clip's slots),
 * hoist_pitch 4 or 8.  The cell threads add sum_j alpha[b][j] * P[b][row][j] (fmaf chain, j ascending) after the K-slice partials and before the bias. */
int l2s_op_skinny_hoist(l2s_model* m, const l2s_skinny_group* group, const float* hoist_p, const float* hoist_alpha, int hoist_pitch, int B, void* stream);

/* One backward GEMM on its own: the operator-level entry of gemm_bwd.hip (tests/test_gemm_bwd_op_gpu.py; lip2speech_amd/native.py op_gemm_bwd).  The
 * descriptor holds the integers of BwdGemmP (l2s_common.h) with the meaning they have there:
 *   mode 0 (DX): C[m][j] = alpha * sum_r dZcol(m, r) * Wp[n(r)][tap(r) * Cin + j]   A = dZ (B,Tz,Nout) rows of lda, B = Wp [Nout][taps*Cin] rows of ldb,
 *                M = B*Tx, N = Cin, K = taps*Nout, padp = taps - 1 - pad (stride 1)
 *   mode 1 (DW): C[n][j] = alpha * sum_m dZ[m][n] * Xcol(m, j)                       A = dZ, B = X (B,Tx,Cin) rows of ldb, M = Nout, N = taps*Cin, K = B*Tz
 *   C rows of ldc; with c_T > 0 row m of C starts at (m / c_T) * c_seq_stride + (m % c_T) * ldc; accumulate: C += instead of C =
 * The 64-bit field comes first, so that the struct has no padding. */
typedef struct l2s_gemm_bwd_desc {
    int64_t c_seq_stride;
    int32_t mode, M, N, K, lda, ldb, ldc, Tx, Tz, taps, stride, pad, padp, Nout, Cin, c_T, accumulate;
    float alpha;
} l2s_gemm_bwd_desc;
/* What one call of a launch function of gemm_bwd.hip ran, as the launch recorder keeps it: entry 0 launch_gemm_bwd, 1 launch_gemm_bwd_splitk,
 * 2 launch_gemm_bwd_dw_dx (then pair = 1, d[0] the DW half and d[1] the DX half; otherwise d[1] is zero); the K slices the caller asked for and the count
 * that ran after clipping to the K tiles (1 = no partial matrices); vec / bf16: the <VEC, BF16> template arguments of the kernel instance; align: the
 * addresses of A, B, C modulo 16 bytes, per descriptor; name: the launch's profile name */
typedef struct l2s_gemm_bwd_record {
    l2s_gemm_bwd_desc d[2];
    int32_t entry, splits_asked, splits, vec, bf16, pair;
    int32_t align[2][3];
    char name[40];
} l2s_gemm_bwd_record;
/* d with its device pointers A, B, C through the product's launch functions and nothing else: d2 == NULL and splits == 0 -> launch_gemm_bwd; d2 == NULL
 * and splits >= 1 -> launch_gemm_bwd_splitk (partials: splits * M * N floats); d2 != NULL -> launch_gemm_bwd_dw_dx with d the DW half, d2 (A2, B2, C2) the
 * DX half and `splits` slices of the DW reduction.  bf16 != 0: bf16 operands (what option "train_bf16" runs).  ran (may be NULL) receives the record of
 * the call - zeroes when the launch was refused; a refused launch returns non-zero with the rule in l2s_last_error */
int l2s_op_gemm_bwd(const l2s_gemm_bwd_desc* d, const float* A, const float* B, float* C, const l2s_gemm_bwd_desc* d2, const float* A2, const float* B2,
                    float* C2, int splits, float* partials, int bf16, l2s_gemm_bwd_record* ran, void* stream);
/* The launch recorder of gemm_bwd.hip (host code, one mutex): cmd 1 = forget what was recorded and arm - from then on every call of the three launch
 * functions, from any entry point of this library, appends its record; cmd 0 = disarm (the records stay); cmd 2 = copy the first `cap` records to out.
 * *count (may be NULL) receives the number of records held */
int l2s_op_gemm_bwd_recorder(int cmd, l2s_gemm_bwd_record* out, int cap, int* count);
/* The carrier of the per-clip tables (csrc/host_table.h) alone: dst[0 .. n) = host_words[0 .. n) on the stream, through kernel arguments, L2S_TABLE_CHUNK
 * words per launch.  host_words may be freed or overwritten as soon as the call returns */
#define L2S_TABLE_CHUNK 960
int l2s_op_upload_table(const int32_t* host_words, int64_t n, int32_t* dst, void* stream);
/* The table builder of csrc/host_table.h on a two-segment table: n_a int32 words, then n_b int64 values (aligned to 8 bytes).  Returns the segments' word
 * offsets and the total; fill == 0 is the sizers' mode (no data read; dst must be NULL); with dst the built table is uploaded through the carrier */
int l2s_op_table_layout(const int32_t* a, int64_t n_a, const int64_t* b, int64_t n_b, int fill, int32_t* dst, int64_t* off_a, int64_t* off_b, int64_t* words,
                        void* stream);
/* The matrices of the post-net's Winograd F(4,5) route (csrc/post_wino.h; option "post_wino"), row-major doubles: AT (4 x 8), G (8 x 5), BT (8 x 8), with
 * AT ((G g) * (BT d)) = the four outputs y[i] = sum_k g[k] d[i + k] of a 5-tap filter over an 8-frame tile.  Pure host code: no device is touched */
int l2s_op_post_wino_matrices(double* AT, double* G, double* BT);
/* The entropy decoder of csrc/jpeg_decode.hip on the HOST: the host instantiation of the one __host__ __device__ function the entropy kernel runs per lane, over
 * the records and table sets of l2s_jpeg_plan; streams (4-byte aligned) is a HOST buffer here.  coefs (16-byte aligned, coef_count int16): per image its
 * blocks x 64 quantised coefficients, image after image - per component a plane of whole MCUs, 64 int16 per block in natural order, the workspace layout;
 * status (n): the word l2s_jpeg_decode reports.  Corrupt streams are tested through this entry point alone: no device is touched */
int l2s_op_jpeg_entropy_host(const uint8_t* streams, int64_t stream_bytes, const l2s_jpeg_image* images, int n, const l2s_jpeg_tables* sets, int n_sets,
                             int16_t* coefs, int64_t coef_count, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* L2S_DIAG_H */
