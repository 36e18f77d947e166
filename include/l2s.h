/*
 * l2s.h - C-ABI of the MI355X-native Lip2Speech hot path (libl2s_hip.so).
 *
 * This is the drop-in boundary.  The reference has no native code:
 * its hot path is the Python call chain
 *
 *     Lip2Speech.inference            /root/reference/model/model.py:43-59
 *       VideoExtractor.forward        /root/reference/model/modules/video.py:76-87
 *       Decoder.inference             /root/reference/model/modules/decoder.py:382-444
 *     Lip2Speech.forward (eval)       /root/reference/model/model.py:23-40
 *       Decoder.forward               /root/reference/model/modules/decoder.py:320-379
 *
 * and a binding for this library replaces the bodies of exactly those methods
 * (INTEGRATION.md shows the ctypes stub a maintainer of the reference would add).
 *
 * Conventions
 *   - plain pointers and sizes only; no framework types.  `stream` is a hipStream_t
 *     passed as void* (NULL = the default stream).  Every entry point only enqueues
 *     work on `stream`; nothing synchronises the device.
 *   - all tensors are fp32, contiguous; "dev" = device memory, "host" = host memory.
 *   - the caller owns every buffer, including the workspace; the library allocates
 *     nothing persistent except the packed weight blob owned by an l2s_model, freed by
 *     l2s_model_destroy.
 *   - every function returns 0 on success, non-zero on error; l2s_last_error() gives
 *     the message for the calling thread.
 *   - lengths are ignored exactly as in the reference (no key masking, zero-padded
 *     frames are encoded and attended like real ones; decoder.py:320-379) - except by
 *     the *_masked entry points ("per-clip video lengths" below), which are opt-in.
 */
#ifndef L2S_H
#define L2S_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct l2s_model l2s_model;

/* fixed geometry of the path (reference/hparams.py, decoder.py:285-318, video.py:55-72) */
#define L2S_N_MELS      80
#define L2S_D_MODEL     512
#define L2S_D_FEAT      768
#define L2S_D_EMB       256
#define L2S_D_VIS       1024
#define L2S_VOCAB       501
#define L2S_MAX_STEPS   300

int         l2s_abi_version(void);
const char* l2s_last_error(void);

/* ---- weights: replaces nn.Module.load_state_dict for encoder.* / decoder.* keys -------------------
 * A model may hold the encoder.* keys, the decoder.* keys, or both (net.encoder / net.decoder are usable on
 * their own in the reference); a stage whose half is absent returns an error.
 * (the on-disk format is the reference's state_dict; demo.py:30-38, evaluate.py:73-77).
 * set_tensor copies `numel` floats from host memory under the checkpoint key (e.g.
 * "decoder.K.0.conv.3.0.weight"); finalize validates that every key of the path is present with the
 * right element count, derives BatchNorm scale/shift, re-lays the weights out for the kernels
 * and uploads one device blob. */
int l2s_model_create(l2s_model** out);
int l2s_model_set_tensor(l2s_model* m, const char* key, const float* host_data, int64_t numel);
int l2s_model_finalize(l2s_model* m, void* stream);
int l2s_model_destroy(l2s_model* m);

/* ---- sizes ---------------------------------------------------------------------------------------- */
/* number of content slots min_T of Content.encode (decoder.py:239-246): min over the strided branches */
int     l2s_min_T(int T);
/* bytes of caller-provided device workspace for one call at these sizes (S = decode steps) */
int64_t l2s_workspace_bytes(int B, int T, int H, int W, int S);
/* floats in the decoder state buffer produced by l2s_decoder_prologue */
int64_t l2s_state_floats(int B, int T);
/* float offset of a field inside the state buffer; layouts:
 *   L2S_ST_K      (B,T,512)   keys,   k[b][t][c]  (the reference holds (B,512,T))
 *   L2S_ST_V      (B,T,512)   values
 *   L2S_ST_CKEY   (B,m,256)   content keys   (reference: self.key (B,256,m))
 *   L2S_ST_CVAL   (B,m,256)   content values (reference: self.value)
 *   L2S_ST_ECELL  (B,512)     encoder_cell
 *   L2S_ST_H / L2S_ST_C   decoder LSTM state, 2 layers, fragment layout
 *   L2S_ST_ENC    (B,T,512)   encoder_outputs after encoder_proj + site + residual
 *   L2S_ST_VP     (B,T,256)   V' = values W_ap^T + b_ap: attention_proj (decoder.py:420) applied to the values once, so that the step's
 *                             a @ V' IS attention_proj(a @ v) (the attention weights sum to one)
 *   L2S_ST_CP     (B,2048,p)  P = content values W_ih0[:, content]^T, the content columns of LSTM layer 0 applied to the values once: rows in the packed
 *                             order 4 * unit + gate, slot j fastest at pitch p = m rounded up to 4 (zeros past m).  Clips of at most 8 content slots
 *                             (T <= 62); longer clips have no table (the field is empty) */
enum { L2S_ST_K = 0, L2S_ST_V = 1, L2S_ST_CKEY = 2, L2S_ST_CVAL = 3, L2S_ST_ECELL = 4,
       L2S_ST_H = 5, L2S_ST_C = 6, L2S_ST_ENC = 7, L2S_ST_STOPC = 8, L2S_ST_VP = 9, L2S_ST_CP = 10 };
int64_t l2s_state_offset(int B, int T, int field);

/* ---- stages ---------------------------------------------------------------------------------------- */
/* Data boundary on the device (datasets/lrw/dataset.py:83-86,123-146 + datasets/__init__.py:7-46, the model-facing half): the decoded
 * uint8 RGB frames of B clips, packed back to back in ONE device buffer (clip i = frames[i] x H x W x 3 bytes at packed_u8 + offsets[i],
 * offsets multiples of 4; both tables are HOST arrays of B entries), become the model's input video dev (B,3,T,H,W) fp32:
 * x/255, then (x - mean_c)/std_c with the ImageNet constants, clips shorter than T zero-padded.  Same fp32 operations in the same order
 * as the reference's host transforms: bit-identical, at a quarter of the PCIe bytes. */
int l2s_normalise_pad_frames(const uint8_t* packed_u8, const int64_t* offsets, const int32_t* frames, int B, int T, int H, int W,
                             float* video, void* stream);

/* The audio half of the same boundary (datasets/spectograms.py:41-59: torchaudio MelSpectrogram - hann window, centre / reflect padding, power 2 -
 * then log(clamp(x, 1e-5)); datasets/__init__.py:7-46: the audio / mel / gate padding of the collates): B waveforms packed back to back in ONE device
 * buffer become the padded log-mel targets, the gates, the mel lengths and the zero-padded audio, in one launch chain (mel_targets.hip).  torchaudio is
 * absent from the build image: the transform is the algorithm as restated in lip2speech_amd/datasets/spectrograms.py - PARITY UNPINNED against the package,
 * like the vocoder below; the kernel is tested against that restatement in fp64.
 * l2s_mel_frames: the frames torch.stft(center=True) makes of n samples at hop 256, n / 256 + 1; 0 and an error for n < 513 (reflect padding of 512
 *   needs n > 512) or n > 2^30.
 * l2s_mel_targets:
 *   audio_packed dev fp32; clip b starts at float offset offsets[b] and has n_samples[b] samples (both HOST arrays of B entries, like the frame tables
 *                above; they may be freed when the call returns).  Any offset works; clips that start on 8-byte boundaries are read with 8-byte loads
 *   fb           dev fp32 (513, n_mels) dense filterbank, fb_nnz its non-zero count (exact, host-side; at most 2048) - the caller's definition of the mel
 *                scale, as l2s_inverse_mel takes it
 *   mels         dev (B, n_mels, M_pad): frame t < l2s_mel_frames(n_b) = log(max(mel_power, 1e-5)) if log_output else mel_power, mel_power = sum over the
 *                band's bins, ascending, of |STFT|^2 fb (fp32; the log is the fp64 one rounded to nearest); frames past it = mel_pad
 *   gate         dev (B, M_pad) or NULL: 0 before frame M_b - 1, 1 from it on
 *   audio_pad    dev (B, A_pad) or NULL: the samples, then zeros
 *   mel_lengths  dev (B) int64 or NULL: M_b
 * Every element of every given output is written.  One 64-lane wave per frame: a frame's values are the same bits whatever else is in the call.
 * Built for n_fft = win_length = 1024 and hop = 256 (what l2s_griffin_lim supports), 1 <= n_mels <= 128, 513 <= n_b <= 2^30, M_pad >= max M_b,
 * A_pad >= max n_b where audio_pad is given; anything else is an error that names the argument, raised before anything is launched. */
int     l2s_mel_frames(int64_t n_samples);
int64_t l2s_mel_targets_workspace_bytes(int B, int n_mels);
int l2s_mel_targets(const float* audio_packed, const int64_t* offsets, const int64_t* n_samples, int B, const float* fb, int fb_nnz, int n_mels,
                    int n_fft, int hop, int log_output, float mel_pad, int M_pad, int64_t A_pad, float* mels, float* gate, float* audio_pad,
                    int64_t* mel_lengths, void* ws, int64_t ws_bytes, void* stream);

/* The face crops of the same boundary (datasets/grid/dataset.py:216-236 and its avspeech / wild twins; LRW's face crops, datasets/lrw/dataset.py:76-79): every
 * frame of those loaders yields one aligned face of its OWN size; two drawn faces go through Resize((160,160)) and (x - 127.5) / 128 to the face tower, and the
 * lower half of every face goes through Resize((96,96)), / 255 and the ImageNet Normalize to the model (frame_resize.hip).  torchvision is absent from the build
 * image: the resize is its published tensor path as lip2speech_amd/datasets/lrw.py::face_recog_resize restates it - PARITY UNPINNED against the package.
 *   packed_u8   dev: n uint8 RGB images, interleaved (H_i, W_i, 3), packed back to back, each starting on a 4-byte boundary; packed_bytes the buffer's size.
 *               No byte outside [0, packed_bytes) is read, and none outside an image's own span rounded out to 4-byte boundaries
 *   jobs        HOST array of n entries that may be freed on return: image (offset, H, W), source rectangle {y0, x0, h, w} inside it, flip (0 / 1: mirror the
 *               rectangle's columns, then resize) and the output slot
 *   mode        L2S_RESIZE_MOUTH: out dev (B,3,T,oh,ow), oh = ow in {96, 88}, slot = b T + t, value = ((u / 255) - mean_c) / std_c - the three operations of
 *               l2s_normalise_pad_frames, the same bits for the same uint8 u.  L2S_RESIZE_FACE: out dev (B,2,3,160,160) as l2s_face_encoder_fwd reads it,
 *               T = 2, slot = 2 b + k, value = (u - 127.5) / 128
 *   u           bilinear, half-pixel centres, no antialias, fp32: src = (h / oh) (dst + 0.5) - 0.5 clamped at 0, the upper tap clamped at the rectangle's last
 *               row / column; rounded half-to-even and clamped to [0, 255]
 * Every element of out is written: a slot that no job names is exact zeros (the zero padding the *_masked entry points ask for).  A slot's bits do not depend on
 * what else is in the call.  The table reaches the device in kernel arguments, L2S_RESIZE_JOBS_PER_LAUNCH slots per launch: no allocation, no synchronisation,
 * no workspace.
 * l2s_resize_check is the pure host check l2s_resize_normalise runs before anything is launched; its error names the job and the limit: offset not a multiple
 * of 4 or image outside [0, packed_bytes); H or W outside [1, 4096]; rectangle empty or outside its image; flip not 0 / 1; slot outside [0, B T) or named
 * twice; a mode or output size that is not built; B T above 2^24. */
typedef struct l2s_resize_job { int64_t offset; int32_t H, W, y0, x0, h, w, flip, slot; } l2s_resize_job;
enum { L2S_RESIZE_MOUTH = 0, L2S_RESIZE_FACE = 1 };
#define L2S_RESIZE_JOBS_PER_LAUNCH 240
int l2s_resize_check(const l2s_resize_job* jobs, int n, int64_t packed_bytes, int mode, int B, int T, int oh, int ow);
int l2s_resize_normalise(const uint8_t* packed_u8, int64_t packed_bytes, const l2s_resize_job* jobs, int n, int mode, int B, int T, int oh, int ow,
                         float* out, void* stream);

/* Face alignment, the step before those crops (datasets/face_utils.py:12-103, called per frame at datasets/grid/dataset.py:216 and its avspeech / wild twins): the
 * face box cut out of the frame is rotated about its centre by the angle of the eye line, with cv2.getRotationMatrix2D and cv2.warpAffine (face_align.hip).
 * OpenCV is absent from the build image: the transform is the fixed-point bilinear path of OpenCV 4.x's generic warpAffine (INTER_LINEAR, constant border 0) as
 * lip2speech_amd/datasets/face_utils.py::warp_affine_u8 restates it - PARITY UNPINNED against the package.  The kernel and that restatement agree to the bit.
 *   packed_in   dev: uint8 RGB images in the layout l2s_resize_normalise reads (interleaved (H_i, W_i, 3), each starting on a 4-byte boundary), packed_bytes the
 *               buffer's size.  No byte outside [0, packed_bytes) is read, and none outside an image's own span rounded out to 4-byte boundaries
 *   packed_out  dev, packed_bytes too, not overlapping packed_in: a job's result goes to the SAME offset, so the job tables of l2s_resize_normalise apply to it
 *               unchanged.  A job writes its image's span rounded up to 4 bytes (clipped to the buffer), the pad bytes as zeros; bytes outside every named span
 *               are left untouched
 *   jobs        HOST array of n entries that may be freed on return: image (offset, H, W) and the six float64 m of its destination-to-source map, source
 *               x = m0 x + m1 y + m2, source y = m3 x + m4 y + m5 (for a rotation: datasets/face_utils.py::rotation_inverse_map).  Output pixel (x, y), with rn =
 *               float64 to the nearest integer, ties to even, each product and sum rounded on its own:
 *                 X = (rn((m1 y + m2) 1024) + 16 + rn(m0 x 1024)) >> 5, Y = (rn((m4 y + m5) 1024) + 16 + rn(m3 x 1024)) >> 5, arithmetic shifts,
 *                 sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31, weights 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy,
 *                 out = (w00 s[sy][sx] + w01 s[sy][sx+1] + w10 s[sy+1][sx] + w11 s[sy+1][sx+1] + 16384) >> 15 per channel, a tap outside the image counting 0
 * An image's output bytes do not depend on what else is in the call.  The table reaches the device in kernel arguments, L2S_ALIGN_JOBS_PER_LAUNCH jobs per launch
 * in table order: no allocation, no synchronisation, no workspace; it works under stream capture.
 * l2s_align_check is the pure host check l2s_align_faces runs before anything is launched; its error names the job and the limit: offset negative or not a
 * multiple of 4; image outside [0, packed_bytes); H or W outside [1, 4096]; a non-finite m; a map that sends a corner of the output outside [-16384, 16384] in
 * either coordinate (inside that, every integer above fits 32 bits, and OpenCV's saturation to short never acts); two jobs whose spans, rounded up to 4 bytes,
 * overlap.  l2s_align_faces also refuses overlapping packed_in / packed_out ranges and pointers off a 4-byte boundary. */
typedef struct l2s_align_job { int64_t offset; int32_t H, W; double m[6]; } l2s_align_job;
#define L2S_ALIGN_JOBS_PER_LAUNCH 56
int l2s_align_check(const l2s_align_job* jobs, int n, int64_t packed_bytes);
int l2s_align_faces(const uint8_t* packed_in, int64_t packed_bytes, const l2s_align_job* jobs, int n, uint8_t* packed_out, void* stream);

/* JPEG decoding, the step before all of the above for the loaders whose frames are stored compressed (datasets/lrw/dataset.py:62-70 and the in-the-wild loader:
 * bz2 pickles of JPEG byte strings, decoded with cv2.imdecode per frame on the host): the compressed strings are uploaded as they are and decoded on the device
 * (jpeg_decode.hip).  libjpeg's default decoder is integer arithmetic throughout - jidctint "islow" IDCT, triangle ("fancy") chroma upsampling, fixed-point
 * YCbCr -> RGB - and lip2speech_amd/datasets/jpeg.py restates it: Pillow / libjpeg-turbo is PINNED against that restatement bit for bit, and the kernels agree
 * with it to the bit; parity with cv2.imdecode stays UNPINNED (OpenCV is absent from the build image).
 * The subset: baseline sequential (SOF0), 8-bit samples, 8-bit quantisation tables, ONE interleaved scan of one component (grey: R = G = B) or of three read as
 * YCbCr with sampling 2x2 / 1x1 / 1x1 (4:2:0) or all 1x1 (4:4:4); restart intervals (DRI / RSTn); H and W in [1, 4096].
 * l2s_jpeg_plan (pure host): n streams in ONE host buffer, stream i the sizes[i] bytes at offsets[i].  Per image its record: the span of the entropy-coded data
 *   (scan_offset, absolute in the buffer; scan_bytes, up to the marker that ends it; eoi = 1 if that marker is EOI), H, W, layout, the restart interval in MCUs and
 *   the index of its TABLE SET.  A table set is what the scan's components use - per component its 64 quantisers in natural order and its DC / AC table ids, and
 *   per Huffman table the derived lookup the kernel wants (lut: the 8-bit window -> length << 8 | symbol, 0 where the code is longer; maxcode / valoff per length
 *   for those; the values) - deduplicated across the call by content into sets[0 .. *n_sets); sets_cap is the room (n always suffices).  Refused, with
 *   "image i" and the reason, before anything else happens: progressive (SOF2), extended (SOF1), lossless and arithmetic-coded frames; 12-bit samples; 16-bit
 *   quantisation tables; four components; other sampling factors; more than one scan; DNL; an Adobe APP14 marker with transform 0 or component ids R, G, B; a
 *   table that the scan names and nothing defined; a header that runs past the stream; H or W outside [1, 4096].  A stream that stops inside its scan is NOT
 *   refused: eoi = 0, and the decode reports it in status.
 * l2s_jpeg_workspace_bytes: the workspace of a decode call of these records (-1 and an error for records l2s_jpeg_decode would refuse).
 * l2s_jpeg_decode:
 *   streams      dev: the compressed streams in one buffer, exactly as planned (4-byte aligned base); stream_bytes its size.  No byte outside
 *                [0, stream_bytes) is read, and of the buffer only the images' scan spans rounded out to 4-byte boundaries
 *   images, sets HOST arrays (the plan's, or the caller's own: every field is checked) that may be freed on return; out_offsets HOST (n) likewise
 *   packed_out   dev: image i is written as interleaved (H_i, W_i, 3) uint8 at out_offsets[i], a multiple of 4 - the layout l2s_normalise_pad_frames,
 *                l2s_resize_normalise and l2s_align_faces read, so a clip of T frames is T images at consecutive offsets.  An image writes its span rounded up
 *                to 4 bytes (clipped to the buffer), the pad bytes as zeros; every other byte of packed_out is left untouched; none outside [0, packed_bytes)
 *                is written
 *   status       dev (n) int32 or NULL: 0 for a stream that decoded cleanly, else the OR of L2S_JPEG_STATUS_*: a bit pattern that is no Huffman code; data that
 *                ends (at the span's end, or at a marker) before the last block, or no EOI after the scan; a restart marker that is missing or out of
 *                sequence; a coefficient run past the end of its block; whole bytes of data left over after the last block of the image or of a restart
 *                interval.  The pixels of such an image are unspecified, and in bounds
 * An image's bytes do not depend on what else is in the call.  Every loop of the kernels is bounded by counts from the records, never by the data.  The records,
 * the table sets and the work list reach the device through the workspace, written in stream order from kernel arguments (the carrier of csrc/host_table.h: a
 * table set alone is 4 040 bytes, the 4 KB of arguments hold none next to anything else): no allocation, no host synchronisation, no copy from host memory; it
 * works under stream capture.  Refused on the host before anything is launched, with the image and the limit: a record outside the ranges above or outside the
 * stream buffer; an output offset that is negative, no multiple of 4 or whose image does not fit packed_bytes; two output spans that overlap (rounded up to 4
 * bytes); stream buffer, packed_out, status and workspace that overlap one another; a workspace smaller than l2s_jpeg_workspace_bytes. */
typedef struct l2s_jpeg_image { int64_t scan_offset; int32_t scan_bytes, H, W, layout, restart, table_set, eoi, reserved; } l2s_jpeg_image;
typedef struct l2s_jpeg_huff { uint16_t lut[256]; int32_t maxcode[18]; int32_t valoff[18]; uint8_t vals[256]; } l2s_jpeg_huff;
/* quant[c]: component c's quantisers, natural order; dc[c] / ac[c]: its table ids (0 / 1); huff[id] the DC tables, huff[2 + id] the AC tables */
typedef struct l2s_jpeg_tables { uint16_t quant[3][64]; uint8_t dc[4], ac[4]; l2s_jpeg_huff huff[4]; } l2s_jpeg_tables;
enum { L2S_JPEG_GREY = 0, L2S_JPEG_444 = 1, L2S_JPEG_420 = 2 };
enum { L2S_JPEG_STATUS_CODE = 1, L2S_JPEG_STATUS_END = 2, L2S_JPEG_STATUS_RESTART = 4, L2S_JPEG_STATUS_RUN = 8, L2S_JPEG_STATUS_EXTRA = 16 };
int l2s_jpeg_plan(const uint8_t* streams, const int64_t* offsets, const int64_t* sizes, int n, l2s_jpeg_image* images, l2s_jpeg_tables* sets, int sets_cap,
                  int* n_sets);
int64_t l2s_jpeg_workspace_bytes(const l2s_jpeg_image* images, int n, int n_sets);
int l2s_jpeg_decode(const uint8_t* streams, int64_t stream_bytes, const l2s_jpeg_image* images, int n, const l2s_jpeg_tables* sets, int n_sets,
                    const int64_t* out_offsets, uint8_t* packed_out, int64_t packed_bytes, int32_t* status, void* ws, int64_t ws_bytes, void* stream);

/* VideoExtractor.forward (video.py:76-87): video dev (B,3,T,H,W) -> feat dev (B,T,768), L2-normalised.
 * H = W in {88, 96}. */
int l2s_encoder_fwd(l2s_model* m, const float* video, int B, int T, int H, int W,
                    float* feat, void* ws, int64_t ws_bytes, void* stream);

/* model.py:52-55: vis[b][t] = cat(feat[b][t] (768), emb[b] (256)) -> dev (B,T,1024) */
int l2s_build_visual(const float* feat, const float* emb, int B, int T, float* vis, void* stream);

/* Decoder prologue (decoder.py:383-410 / 321-351): vis dev (B,T,1024) = the `encoder_outputs` argument
 * of Decoder.forward/inference, emb dev (B,256) = its `face_features[:, 0]`, gumbel dev (B*min_T,501) =
 * the noise F.gumbel_softmax would draw (decoder.py:257).  Writes the state buffer and content_dis dev
 * (B*min_T,501) (softmax of the content logits, the 6th output of Decoder.forward; may be NULL). */
int l2s_decoder_prologue(l2s_model* m, const float* vis, const float* emb, const float* gumbel,
                         int B, int T, float* state, float* content_dis,
                         void* ws, int64_t ws_bytes, void* stream);

/* The autoregressive loop (decoder.py:412-429 / 353-375), S steps from the state buffer.
 *   teacher      dev (B,S,80) or NULL: frame fed at step i when teacher_mask[i] != 0
 *                (= cat(BOS, mels)[:, i], decoder.py:349,357)
 *   teacher_mask host (S) bytes or NULL: the scheduled-sampling decisions, made by the caller
 *   mel          dev (B,S,80)  pre-postnet frames, channel-last
 *   stop         dev (B,S)     stop-token logits
 *   attn         dev (B,S,T) or NULL; post-softmax weights, or tau*q.k logits if attn_logits != 0
 *                (inference() returns the former, forward() the latter) */
int l2s_decode_steps(l2s_model* m, float* state, int B, int T, int S,
                     const float* teacher, const uint8_t* teacher_mask,
                     float* mel, float* stop, float* attn, int attn_logits,
                     void* ws, int64_t ws_bytes, void* stream);

/* Postnet + residual (decoder.py:143-156, 438-439): mel dev (B,S,80) -> mel_post dev (B,80,S) in the
 * reference's layout; mel_cf dev (B,80,S) or NULL additionally receives the transposed pre-postnet mel. */
int l2s_postnet(l2s_model* m, const float* mel, int B, int S, float* mel_post, float* mel_cf,
                void* ws, int64_t ws_bytes, void* stream);

/* SpeakerEncoder.inference (model/modules/audio.py:131-150; called at demo.py:84): audio dev (B, n_samples) 16 kHz ->
 * 40-band mel power spectrogram (n_fft 400, hop 160, hann, centre/reflect, HTK, no log) -> 3 x LSTM(256) ->
 * Linear(last hidden) -> ReLU -> L2 normalise -> emb dev (B,256).  Needs the speaker_encoder.* keys in the model.
 * n_samples > 200 (the reflect padding) and ws_bytes >= l2s_speaker_workspace_bytes(B, n_samples), else the call fails before it launches anything. */
int64_t l2s_speaker_workspace_bytes(int B, int n_samples);
int l2s_speaker_encoder_fwd(l2s_model* m, const float* audio, int B, int n_samples, float* emb,
                            void* ws, int64_t ws_bytes, void* stream);

/* The same tower over B clips of UNEQUAL length: emb dev (B,256), row b (call order) = what l2s_speaker_encoder_fwd returns for clip b alone at
 * B = 1, n_samples = n_samples[b].  audio_packed dev fp32: clip b is the n_samples[b] floats at float offset offsets[b] (any offset; no alignment
 * asked); nothing outside [offsets[b], offsets[b] + n_samples[b]) is read, so a zero-padded (B, N) tensor is the special case offsets[b] = b * N
 * and what pads it never matters.  offsets / n_samples are HOST int64 arrays that may be freed on return (as in l2s_mel_targets).
 * Limits: n_samples[b] in [201, 2^30]; 1 <= B <= L2S_SPK_MAX_CLIPS and R = sum L_b <= L2S_SPK_MAX_ROWS, L_b = n_samples[b] / 160 + 1 - the row
 * counts l2s_speaker_encoder_fwd itself can launch (it states no limit: its recurrence puts ceil(B / 16) row tiles and its GEMMs ceil(B L / 64) in
 * the grid's y dimension, 65 535 at the most).  A violation is an error naming the row, raised before anything is launched; emb is then untouched.
 * Rows: the time-major compact layout (torch's PackedSequence) - clips ranked by L_b descending, ties in call order; frame l of the clip of rank r
 * is row step_row0[l] + r of R.  l2s_speaker_packed_plan is that layout as a pure host function: order[B] (rank -> clip), step_rows[L_max]
 * (clips with L_b > t), step_row0[L_max + 1] (its prefix sum), L_max, R; size the three arrays for max n_samples / 160 + 2 entries.
 * Bits: every kernel is row-wise; where R and the step row counts pick the kernel forms of the solo call (R < 3 969 and B <= 96 under the
 * defaults) the embedding has the solo call's bits, elsewhere it agrees to rounding.
 * l2s_speaker_workspace_bytes_packed is sized from the R compact rows; -1 (with l2s_last_error) outside the limits. */
#define L2S_SPK_MAX_CLIPS 1048560
#define L2S_SPK_MAX_ROWS 4194240
int l2s_speaker_packed_plan(const int64_t* n_samples, int B, int32_t* order, int32_t* step_rows, int32_t* step_row0, int* L_max, int64_t* R);
int64_t l2s_speaker_workspace_bytes_packed(const int64_t* n_samples, int B);
int l2s_speaker_encoder_packed(l2s_model* m, const float* audio_packed, const int64_t* offsets, const int64_t* n_samples, int B, float* emb,
                               void* ws, int64_t ws_bytes, void* stream);

/* face speaker tower: FaceRecognizer (reference vgg_face.py:28-60), facenet_pytorch's InceptionResnetV1 (casia-webface) in eval mode + projection.
 * Needs a model holding the vgg_face.* keys (resnet.* without logits.*, projection_layer.*).  H = W = 160 only (the reference's loaders resize faces
 * to 160); other sizes return an error (the workspace query returns -1).  Runs fp32-exact on the split-bf16 matrix path under every option
 * ("infer_bf16" does not apply to the tower).  A face's outputs have the same bits whatever else is in the batch.
 * faces dev: image b at faces + b*batch_stride floats, (3,H,W) contiguous (the strided face_frames[:, 0] view works as it is)
 * -> proj dev (B,256) the pre-ReLU projection (forward's output; may be NULL), emb dev (B,256) = normalize(relu(proj)) (inference's output) */
int64_t l2s_face_workspace_bytes(int B, int H, int W);
int l2s_face_encoder_fwd(l2s_model* m, const float* faces, int64_t batch_stride, int B, int H, int W,
                         float* proj, float* emb, void* ws, int64_t ws_bytes, void* stream);

/* ---- vocoder + metric of evaluate.py -------------------------------------------------------------
 * The reference vocodes the predicted mels with torchaudio 0.9.0 (datasets/spectograms.py:76-95: exp -> InverseMelScale ->
 * GriffinLim, 256 iterations each) and scores them with pystoi 0.3.3 (evaluate.py:41-45: stoi(gt, pred, fs, extended=True)).
 * Both packages are absent from the build image: these entry points run the published algorithms as restated in
 * lip2speech_amd/datasets/spectrograms.py and lip2speech_amd/metrics.py - PARITY UNPINNED against the packages themselves.
 * The random start iterates of both vocoder stages are INPUTS (the reference draws them with torch.rand).
 *
 * l2s_inverse_mel: torchaudio.transforms.InverseMelScale.forward.  mel dev (N, n_mels, L): power mel, or log-mel when log_input
 *   (spectral_de_normalize = exp is then applied on the fly); fb dev (n_freqs, n_mels) with fb_nnz non-zero entries (exact count,
 *   the caller knows its filterbank; at most 2048); init dev (N*L, n_freqs), row n*L + l = the start spectrum of frame l of clip n.
 *   The N clips are N / rows_per_call independent calls (the SGD's 1/(rows*L) gradient scale, the loss mean and the two stopping
 *   rules - loss < 1e-5, |loss - previous loss| < 1e-8, the update of the stopping iteration still applied - are per call).
 *   spec dev (N, n_freqs, L) >= 0.  loss_per_iter dev (calls, iters) or NULL; iters_run dev int (calls) or NULL.
 * l2s_griffin_lim: torchaudio.functional.griffinlim (power 2, rand_init replaced by init_angles dev (N, n_freqs, L, 2) used as
 *   given, momentum 0.99): power_spec dev (N, 513, L) -> wave dev (N, hop*(L-1)).  n_fft = win_length = 1024, hop = 256, L >= 5.
 *   Up to 121 frames (1.9 s) the clip's waveform stays in one block's LDS for the whole loop: one launch.  From 122 frames on, one launch
 *   per iteration over (clip, tile of 24 frames): a block recomputes the samples its frames read (a halo of three frames each side) and
 *   the rebuilt spectra rotate through three workspace slots - l2s_griffin_lim_workspace_bytes grows from two to three slots there, about
 *   14.6 KB per frame (140 MB at N = 32, L = 300); any L the workspace allows.  Either way a clip's waveform depends on neither N nor its
 *   neighbours.
 * l2s_estoi: pystoi.stoi(clean, pred, fs, extended=True) per clip: clean / pred dev (N, n_samples); fir dev = the polyphase
 *   resampling filter of scipy.signal.resample_poly(x, up, down) INCLUDING its leading zero pad (n_fir taps, already scaled by up),
 *   n_pre_remove / n_resampled as resample_poly computes them, or fir = NULL when fs is already 10 kHz; band_lo_hi_host = HOST
 *   array of 2 x 15 ints, first / last+1 bin of each one-third octave band; score dev (N).  Up to 16 512 resampled samples (1.65 s)
 *   both signals stay in one block's LDS; above that, up to 48 256 (4.8 s), they live in the workspace and the resampler is a kernel of
 *   its own - the same algorithm and order of sums.  l2s_estoi_workspace_bytes_long sizes the workspace of the form a call takes
 *   (= l2s_estoi_workspace_bytes(N) up to 16 512 samples); l2s_estoi checks ws_bytes against it. */
int64_t l2s_inverse_mel_workspace_bytes(int N, int L, int n_mels, int n_freqs, int rows_per_call, int iters);
int l2s_inverse_mel(const float* mel, int log_input, const float* fb, int fb_nnz, const float* init, int N, int L, int n_mels, int n_freqs,
                    int rows_per_call, int iters, float* spec, float* loss_per_iter, int* iters_run, void* ws, int64_t ws_bytes, void* stream);
int64_t l2s_griffin_lim_workspace_bytes(int N, int L);
int l2s_griffin_lim(const float* power_spec, const float* init_angles, int N, int L, int n_fft, int hop, int iters, float momentum,
                    float* wave, void* ws, int64_t ws_bytes, void* stream);
int64_t l2s_estoi_workspace_bytes(int N);
int64_t l2s_estoi_workspace_bytes_long(int N, int n_resampled);
int l2s_estoi(const float* clean, const float* pred, int N, int n_samples, const float* fir, int n_fir, int up, int down, int n_pre_remove,
              int n_resampled, const int* band_lo_hi_host, float* score, void* ws, int64_t ws_bytes, void* stream);

/* The same three stages over N clips of UNEQUAL length in one launch chain: every clip comes out as the entry point above computes it ALONE at its own length
 * (N = 1, L = L_b, rows_per_call = 1; N = 1, n_samples = n_samples[b]) - the same bits, whatever shares the call and in whatever order.  PARITY UNPINNED against
 * torchaudio and pystoi, as above.  L / n_samples / n_fir / n_resampled / mel_offset / mel_pitch are HOST arrays of N entries that may be freed on return.
 * One layout rule between the stages: clips back to back in clip order, clip b's block exactly the array its solo call uses, block offsets the prefix sums of
 * L_b - init (L_b, n_freqs) at row sum_{c<b} L_c, spec (n_freqs, L_b) and init_angles (513, L_b, 2) at frame offset sum_{c<b} L_c.  The mel input is the
 * exception, so that the packed blocks l2s_forward_eval_ragged writes and a padded (N, n_mels, L_max) tensor are both read in place: band m, frame l of clip b
 * is mel[mel_offset[b] + m mel_pitch[b] + l] (floats from one base pointer of mel_floats floats; frames past L_b are never read).
 * l2s_inverse_mel_ragged: the gradient scale -2 / L_b, the loss mean and the two stopping rules run over the clip's own rows, and the second pass re-runs only the
 *   clips that stopped early; loss_per_iter dev (N, iters) or NULL and iters_run dev int (N) or NULL are per clip; the band tables are built once per call.
 * l2s_griffin_lim_ragged: a clip takes the kernel form its solo call takes (up to 77 frames, up to 121, the tile form above): at most two launches for the short
 *   clips plus one launch per iteration over the (clip, tile) pairs of the long clips only.  wave dev (N, wave_pitch): clip b's hop (L_b - 1) samples at the row
 *   start, exact zeros behind them; every element is written.
 * l2s_estoi_ragged: clean / pred dev (N, pitch), clip b its first n_samples[b] floats (nothing behind them is read).  ONE filter table serves the call:
 *   scipy's resample_poly plans for different input lengths differ only in their trailing zeros, so clip b uses the first n_fir[b] taps of fir (n_fir_max taps,
 *   the longest clip's plan) with its own n_resampled[b]; up / down / n_pre_remove do not depend on the length.  fir = NULL (n_fir ignored) when fs is 10 kHz.
 *   A clip takes the short or the long form by its own n_resampled[b].  score dev (N).
 * The tables reach the device through the workspace, written on the stream by a kernel that carries them in its arguments (960 integers per launch): no
 * allocation, no host synchronisation, no copy from host memory.
 * Limits, each refused by the pure host checks l2s_*_ragged_check (which the entry points run before anything is launched; the error names the clip):
 * N in [1, 65 535]; L_b in [5, 2^20] and sum L_b <= 2^24; n_fft = win = 1024, hop = 256; at most 128 mel bands, 576 bins, 2048 filterbank non-zeros;
 * mel_offset[b] >= 0, mel_pitch[b] >= L_b and mel_offset[b] + (n_mels - 1) mel_pitch[b] + L_b <= mel_floats; wave_pitch >= hop (L_b - 1) and pitch >=
 * n_samples[b] (rows that do not overlap); n_resampled[b] in [1, 48 256]; n_fir[b] in [1, n_fir_max].  A null table is refused.
 * The workspace sizers are never below the sum of the solo sizers over the clips and grow with sum L_b; -1 (with l2s_last_error) for a table they refuse. */
int l2s_inverse_mel_ragged_check(const int* L, const int64_t* mel_offset, const int64_t* mel_pitch, int N, int64_t mel_floats, int n_mels, int n_freqs,
                                 int fb_nnz, int iters);
int64_t l2s_inverse_mel_ragged_workspace_bytes(const int* L, int N, int n_mels, int n_freqs, int iters);
int l2s_inverse_mel_ragged(const float* mel, int64_t mel_floats, const int64_t* mel_offset, const int64_t* mel_pitch, const int* L, int N, int log_input,
                           const float* fb, int fb_nnz, const float* init, int n_mels, int n_freqs, int iters, float* spec, float* loss_per_iter,
                           int* iters_run, void* ws, int64_t ws_bytes, void* stream);
int l2s_griffin_lim_ragged_check(const int* L, int N, int n_fft, int hop, int iters, int64_t wave_pitch);
int64_t l2s_griffin_lim_ragged_workspace_bytes(const int* L, int N);
int l2s_griffin_lim_ragged(const float* power_spec, const float* init_angles, const int* L, int N, int n_fft, int hop, int iters, float momentum,
                           float* wave, int64_t wave_pitch, void* ws, int64_t ws_bytes, void* stream);
int l2s_estoi_ragged_check(const int* n_samples, const int* n_fir, const int* n_resampled, int N, int64_t pitch, int has_fir, int n_fir_max, int up, int down,
                           int n_pre_remove);
int64_t l2s_estoi_ragged_workspace_bytes(const int* n_resampled, int N);
int l2s_estoi_ragged(const float* clean, const float* pred, int64_t pitch, const int* n_samples, int N, const float* fir, int n_fir_max, const int* n_fir,
                     int up, int down, int n_pre_remove, const int* n_resampled, const int* band_lo_hi_host, float* score, void* ws, int64_t ws_bytes,
                     void* stream);

/* decoder.py:429-435: lengths[b] = first i+1 with stop logit > 0, else S.  lengths dev (B) int64. */
int l2s_output_lengths(const float* stop, int B, int S, int64_t* lengths, void* stream);

/* Lip2Speech.inference with a supplied speaker embedding (model.py:43-59), all stages on `stream`:
 * mel_post dev (B,80,S), lengths dev (B) int64, attn dev (B,S,T) or NULL. */
int l2s_inference(l2s_model* m, const float* video, const float* emb, const float* gumbel,
                  int B, int T, int H, int W, int S,
                  float* mel_post, int64_t* lengths, float* attn,
                  void* ws, int64_t ws_bytes, void* stream);

/* ---- per-clip video lengths: padded clips decode as they would alone -----------------------------------------------------------------------------
 * The entry points above ignore lengths as the reference does: a clip's speech then depends on what it was padded to.  The *_masked forms take one
 * more argument, `video_lengths`: a HOST array of B int32 (the collate holds the lengths on the host; the library plans its launches from them and
 * carries what the kernels need to the device in kernel arguments on `stream` - the array may be freed when the call returns).
 *
 * Contract.  The batch is B clips ZERO-padded to T: frames t >= len_b of clip b must be EXACTLY 0.0f, as l2s_normalise_pad_frames and the reference's
 * train_collate_fn_pad produce (the front-end's temporal padding is zeros too, which is what makes a padded clip's real frames see what a solo clip
 * sees; non-zero pad frames leak into the last two real frames of a clip).  len_b in [7, T]; anything else is an error (l2s_last_error names the row).
 * Row b of every output is then what the same entry point returns for clip b ALONE at T = len_b - mel_post, the pre-post-net mel, stop logits,
 * output lengths, attention at t < len_b - with the same order of the same fp32 sums wherever the kernel choice does not depend on the row count
 * (DESIGN.md section 8), rounding-level otherwise.  Attention columns t >= len_b are exactly 0; attention LOGITS (l2s_forward_eval_masked,
 * attn_logits != 0) are -INFINITY there, so that the caller's softmax over T (train.py:244) gives those columns exactly 0 as well.
 * Content slots: m_b = l2s_min_T(len_b) <= m = l2s_min_T(T).  Clip b uses the FIRST m_b of its m Gumbel rows (rows b*m .. b*m + m_b - 1 of `gumbel`)
 * and of its m content_dis rows; its other content_dis rows are zeros.
 * State buffer of the staged pair: rows t >= len_b of L2S_ST_ENC are zeros, of L2S_ST_K / _V / _VP unspecified (finite, never read by a masked loop);
 * content keys / values of slots >= m_b unspecified / zero.  A state written by l2s_decoder_prologue_masked goes to l2s_decode_steps_masked with the
 * same lengths.
 * Options: masked calls take the launch-per-phase route - "persist_decode" and "use_graph" do not apply to them - unless "persist_masked" is set
 * (below: free-running masked calls inside the persistent envelope then take the persistent forms); "early_stop", "fold_step_weights" and
 * "infer_bf16" compose.  The grouped (*_multi) entry points have no masked form: batches of unequal length share a launch chain through
 * l2s_inference_ragged and, on the evaluate route, l2s_forward_eval_ragged ("ragged groups" below); the training entry points have their own (l2s_train_*_masked_fwd / _masked_bwd, "training with per-clip video lengths" below).
 * Workspace: l2s_workspace_bytes_masked (the unmasked size plus the device length table), for all four calls.
 * l2s_masked_bilstm_plan: the launch plan of the BiLSTM recurrence, a pure host function.  The recurrence stays T uniform launches (step s reads frame
 * s forward and frame T-1-s backward); capture_steps = the steps AFTER which a row kernel hands over the forward finals of the clips that ended there
 * (s = len_b - 1), reset_steps = the steps BEFORE which a row kernel restarts, from the site embedding, the backward rows of the shorter clips whose
 * last frame is read there (s = T - len_b, len_b < T).  Both ascending without repeats, at most B entries each. */
int64_t l2s_workspace_bytes_masked(int B, int T, int H, int W, int S);
int l2s_masked_bilstm_plan(const int32_t* video_lengths, int B, int T, int32_t* capture_steps, int32_t* reset_steps, int* n_capture, int* n_reset);
int l2s_inference_masked(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S,
                         float* mel_post, int64_t* lengths, float* attn, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths);
int l2s_forward_eval_masked(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S,
                            const float* teacher, const uint8_t* teacher_mask, float* mel_cf, float* mel_post, float* stop, float* attn_logits,
                            float* content_dis, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths);
int l2s_decoder_prologue_masked(l2s_model* m, const float* vis, const float* emb, const float* gumbel, int B, int T, float* state,
                                float* content_dis, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths);
int l2s_decode_steps_masked(l2s_model* m, float* state, int B, int T, int S, const float* teacher, const uint8_t* teacher_mask, float* mel,
                            float* stop, float* attn, int attn_logits, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths);

/* Grouped inference ("advance G independent batches per launch"): G batches of B clips each - separate tensors, wherever the caller's
 * loader put them - run as rows g*B .. g*B+B-1 of ONE launch chain on ONE weight blob: the 300 x 4 step launches, the BiLSTM recurrence and
 * every GEMM are issued once per G batches instead of once per batch, and from M = 64 rows on the batch-row kernels use register-blocked
 * 2x1 / 2x2 / 4x2 tiles (half the operand traffic per row; at M = 128 the LSTM launches are MFMA-bound).  Replaces G passes through the
 * reference's loop (model/modules/decoder.py:412-435) over G DataLoader batches (demo.py:60-90 / evaluate.py:22-51 iterate them one by one).
 * Every kernel of the path is row-independent, so each batch's mel / lengths / attention are bit-identical to l2s_inference on that batch.
 * video[g] dev (B,3,T,H,W), emb[g] dev (B,256), gumbel[g] dev (B*l2s_min_T(T),501) - host arrays of G device pointers;
 * mel_post dev (G*B,80,S), lengths dev (G*B) int64, attn dev (G*B,S,T) or NULL - batch g is the g-th slice of B rows. */
#define L2S_MAX_GROUP 8
int64_t l2s_workspace_bytes_multi(int G, int B, int T, int H, int W, int S);
int l2s_inference_multi(l2s_model* m, int G, const float* const* video, const float* const* emb, const float* const* gumbel,
                        int B, int T, int H, int W, int S,
                        float* mel_post, int64_t* lengths, float* attn,
                        void* ws, int64_t ws_bytes, void* stream);

/* ---- ragged groups: batches of unequal length share one launch chain -------------------------------------------------------------------------------------
 * G padded batches, each with its OWN B_g and T_g (a loader that pads every batch to its longest clip), run as rows of ONE launch chain, every clip
 * decoded as it would be alone, the visual encoder on the real frames only.  Clip c = the c-th clip in batch order (N = sum B_g clips, Tmax = max T_g).
 *   video[g] dev (B_g,3,T_g,H,W), 16-byte aligned, read in place; emb[g] dev (B_g,256); gumbel[g] dev (B_g * l2s_min_T(T_g), 501) - exactly what
 *   l2s_inference_masked takes for that batch alone; batch_B / batch_T host (G); video_lengths host (N), may be freed when the call returns;
 *   mel_post dev (N,80,S), lengths dev (N) int64, attn dev (N,S,Tmax) or NULL.
 * Limits: 1 <= G <= L2S_MAX_GROUP, N <= L2S_MAX_RAGGED_CLIPS, 7 <= len_c <= T_g <= 300 (T_g may exceed its batch's longest clip).  A violation is an
 * error that names the batch and the row (l2s_last_error), raised before anything is launched: the outputs of a failed call are untouched.
 * Contract.  Row c of every output is what l2s_inference_masked gives for that clip - so what l2s_inference gives for the clip alone at T = len_c;
 * attention columns t >= len_c are exactly 0.  The same bits wherever the kernel choice is the same, rounding-level inside the 1e-3
 * gate elsewhere.  The choices that depend on the row count (the split-bf16 GEMM's tile threshold, the post-net's one-slice-per-tap form) are made on the
 * rows of the WHOLE call, as for one masked call of N clips padded to Tmax: "rows of one batch", which the *_multi calls decide on, has no meaning in a
 * ragged group.  Frames t >= len_c of a clip are NEVER READ - the front-end looks its clip up in a table and bounds its temporal taps by len_c - so the
 * zero-padding contract of the *_masked entry points is not needed here: the pad frames may hold anything.
 * Route and options: the launch-per-phase route, like every masked call and every grouped call - never a persistent form, whatever "persist_decode" /
 * "persist_masked" say; "early_stop" and "fold_step_weights" compose; "use_graph" does not apply.  "infer_bf16" set, or "frontend_x3" other than 3, is an
 * error that names the option: the ragged front-end exists in the default form only, and there is no padded copy of the frames to fall back on.
 * l2s_ragged_plan (pure host): frame0[c] / pair0[c] = prefix sums of len_c and of ceil(len_c / 2) over the clips, N + 1 entries each - clip c owns the
 * compact encoder frames frame0[c] .. frame0[c+1] - 1 and the front-end's pair blocks pair0[c] .. pair0[c+1] - 1 (two output frames per block).
 * l2s_workspace_bytes_ragged: the worst case, every frame real; -1 (and l2s_last_error) for shapes outside the limits. */
#define L2S_MAX_RAGGED_CLIPS 256          /* = L2S_MAX_GROUP x 32, the largest row count the grouped route is benchmarked at */
int l2s_ragged_plan(int G, const int32_t* batch_B, const int32_t* batch_T, const int32_t* video_lengths,
                    int32_t* frame0, int32_t* pair0, int* N, int* Tmax);
int64_t l2s_workspace_bytes_ragged(int G, const int32_t* batch_B, const int32_t* batch_T, int H, int W, int S);
int l2s_inference_ragged(l2s_model* m, int G, const float* const* video, const float* const* emb, const float* const* gumbel,
                         const int32_t* batch_B, const int32_t* batch_T, const int32_t* video_lengths,
                         int H, int W, int S, float* mel_post, int64_t* lengths,
                         float* attn, void* ws, int64_t ws_bytes, void* stream);

/* The evaluate-shaped ragged group: Lip2Speech.forward(..., tf_ratio = 1) in eval() mode (evaluate.py:32-38; l2s_forward_eval_masked below) over G padded
 * batches that differ in B_g, T_g AND in their step count S_g = melspecs.shape[2], as rows of ONE launch chain.  Free-running only: there are no teacher
 * frames (at tf_ratio = 1 no step is teacher-forced; a teacher-forced batch keeps its own l2s_forward_eval_masked call).
 *   video / emb / gumbel / batch_B / batch_T / video_lengths: exactly what l2s_inference_ragged takes; batch_S host (G), each in [1, L2S_MAX_STEPS].
 *   Outputs are PACKED back to back in batch order: batch g's block starts at float offset *_off[g] of l2s_forward_eval_ragged_plan and has the layout
 *   l2s_forward_eval_masked gives that batch alone - mel_cf and mel_post (B_g,80,S_g) at mel_off[g]; stop (B_g,S_g) at stop_off[g]; attn_logits
 *   (B_g,S_g,T_g) at attn_off[g], tau * q.k, -INFINITY at columns t >= len_c; content_dis (B_g * l2s_min_T(T_g), 501) at dis_off[g], a clip's rows past
 *   its l2s_min_T(len_c) slots zeros.  mel_cf, attn_logits and content_dis may be NULL.  Each tensor holds *_off[G] floats.
 * Contract.  Batch g's blocks are what l2s_forward_eval_masked(batch g, S = S_g, teacher = NULL) returns: the same bits wherever the kernel choice is the
 * same, rounding-level inside the 1e-3 gate elsewhere.  The choices that depend on the row count (the split-bf16 GEMM's tile threshold, the post-net's
 * one-slice-per-tap form) are made on the rows of the WHOLE call - N * Tmax, N * Smax with Smax = max S_g - as l2s_inference_ragged makes them.  Frames
 * t >= len_c are never read (the ragged front-end as it is).  The chain decodes every row for Smax steps: the steps j >= S_g of a shorter batch's rows are
 * wasted work, and none of them reaches an output - the post-net (five same-padded Conv1d layers over time) sees zeros past every row's own S_g, as it does
 * in the batch's own call, and only frames j < S_g are moved into the blocks.  When every S_g equals Smax nothing has to be zeroed and those launches are
 * skipped.
 * Limits and errors: those of l2s_inference_ragged, plus 1 <= S_g <= L2S_MAX_STEPS; every violation names the batch ("batch 1 has S = 301, outside [1, 300]")
 * and is raised before the first launch - the outputs of a failed call are untouched.  "infer_bf16" set, "frontend_x3" other than 3 and "frontend_solo" are
 * refused by name; "early_stop" (S comes from the target), "persist_*" and "use_graph" do not apply: the launch-per-phase route.
 * l2s_forward_eval_ragged_plan (pure host): the four offset tables, G + 1 entries each, in floats, and N = sum B_g, Tmax, Smax.
 * l2s_workspace_bytes_eval_ragged: l2s_workspace_bytes_ragged at S = Smax plus the staging buffers at pitch Smax / Tmax; -1 (and l2s_last_error) outside the limits. */
int l2s_forward_eval_ragged_plan(int G, const int32_t* batch_B, const int32_t* batch_T, const int32_t* batch_S,
                                 int64_t* mel_off, int64_t* stop_off, int64_t* attn_off, int64_t* dis_off, int* N, int* Tmax, int* Smax);
int64_t l2s_workspace_bytes_eval_ragged(int G, const int32_t* batch_B, const int32_t* batch_T, const int32_t* batch_S, int H, int W);
int l2s_forward_eval_ragged(l2s_model* m, int G, const float* const* video, const float* const* emb, const float* const* gumbel,
                            const int32_t* batch_B, const int32_t* batch_T, const int32_t* batch_S, const int32_t* video_lengths,
                            int H, int W, float* mel_cf, float* mel_post, float* stop, float* attn_logits, float* content_dis,
                            void* ws, int64_t ws_bytes, void* stream);

/* Lip2Speech.forward(..., tf_ratio) in eval() mode (model/model.py:23-40 + model/modules/decoder.py:320-379) - what evaluate.py:32-38 runs on
 * every batch at tf_ratio = 1 - as ONE launch chain: encoder, prologue, S = mels.shape[2] steps, post-net.
 *   teacher      dev (B,S,80) or NULL: cat(BOS, mels)[:, i] (decoder.py:349), fed at the steps whose teacher_mask byte is set
 *   teacher_mask host (S) bytes or NULL: the caller's scheduled-sampling draws (decoder.py:355-357); both or neither
 *   mel_cf       dev (B,80,S) or NULL  pre-postnet mel, the reference's layout (outputs[0])
 *   mel_post     dev (B,80,S)          (outputs[1])
 *   stop         dev (B,S)             stop-token logits (outputs[2] without its trailing 1)
 *   attn_logits  dev (B,S,T) or NULL   tau * q.k, PRE-softmax (outputs[4]; train.py:244 applies the softmax itself)
 *   content_dis  dev (B*min_T,501) or NULL  (outputs[5])
 * Workspace: l2s_workspace_bytes(B,T,H,W,S).  Same kernels as the staged calls l2s_encoder_fwd .. l2s_postnet: bit-identical to them. */
int l2s_forward_eval(l2s_model* m, const float* video, const float* emb, const float* gumbel, int B, int T, int H, int W, int S,
                     const float* teacher, const uint8_t* teacher_mask, float* mel_cf, float* mel_post, float* stop, float* attn_logits,
                     float* content_dis, void* ws, int64_t ws_bytes, void* stream);
/* The grouped form (see l2s_inference_multi): G batches of evaluate.py's loop (evaluate.py:32-38 iterates them one by one) as rows
 * g*B .. g*B+B-1 of ONE launch chain; per batch bit-identical to l2s_forward_eval.  video / emb / gumbel / teacher: host arrays of G device
 * pointers (teacher NULL = free-running).  The batches of a group share S and teacher_mask - at tf_ratio = 1 the mask is empty, so any G
 * batches of one shape group.  Outputs are (G*B, ...) tensors, batch g = the g-th slice of B rows (content_dis: of B*min_T rows).
 * Workspace: l2s_workspace_bytes_multi(G,B,T,H,W,S). */
int l2s_forward_eval_multi(l2s_model* m, int G, const float* const* video, const float* const* emb, const float* const* gumbel,
                           const float* const* teacher, const uint8_t* teacher_mask, int B, int T, int H, int W, int S, float* mel_cf,
                           float* mel_post, float* stop, float* attn_logits, float* content_dis, void* ws, int64_t ws_bytes, void* stream);

/* ---- training-side primitives of the data-parallel step (train.py:102-104,172-193; train_utils/losses.py:69-77) ----------
 * scratch: l2s_train_scratch_bytes() of device memory.  Reductions are two-stage fp64 (deterministic). */
int64_t l2s_train_scratch_bytes(void);
/* losses5 dev = {mel MSE, 10 * post-net mel MSE, gate BCE-with-logits, KLD(content_dis || uniform), sum}; mel/mel_post/mel_target are
 * (B,80,S) channel-first as Decoder.forward returns them, stop/gate (B,S), content_dis (R,501).  d* (may be NULL) receive the
 * gradients of the summed loss. */
int l2s_loss(const float* mel, const float* mel_post, const float* mel_target, const float* stop, const float* gate_target,
             const float* content_dis, int B, int S, int R, float* losses5, float* dmel, float* dmel_post, float* dstop, float* ddis,
             void* scratch, void* stream);
/* norm_out dev [1] = ||grads||_2 over a flat gradient range (torch.nn.utils.clip_grad_norm_'s total norm) */
int l2s_grad_norm(const float* grads, int64_t n, void* scratch, float* norm_out, void* stream);
/* torch.optim.AdamW(amsgrad=True) on a flat range, fused with gradient averaging and clipping:
 * g_eff = grads * grad_mul * min(1, max_norm / (grad_norm[0] * grad_mul + 1e-6)); grad_norm dev [1] or NULL (no clipping).
 * grad_mul = 1/world_size after a sum all-reduce.  step counts from 1. */
int l2s_adamw_amsgrad_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_norm,
                           float grad_mul, float max_norm, void* stream);

/* ---- training path of the model (forward with tapes + backward of encoder, prologue, loop, post-net) ---------------------------
 * l2s_train_bind: device pointers of a parameter in its canonical (checkpoint) layout and of its gradient slot (may be NULL), by key.
 * The backward entry points write parameter gradients into the bound slots (overwrite, not accumulate). */
int l2s_train_bind(l2s_model* m, const char* key, float* param_dev, float* grad_dev);
/* BatchNorm behaviour of the l2s_train_* entry points: batch_stats = 1 -> nn.Module.train() semantics (normalise with the statistics of
 * this batch, update the BOUND running_mean / running_var in place with `momentum`, unbiased running variance; per process - no cross-rank
 * synchronisation, like the single-device reference); 0 (default) -> running statistics (eval()). */
int l2s_train_set_bn(l2s_model* m, int batch_stats, float momentum);
/* After an optimizer step: rebuild the packed blob ON THE DEVICE from the bound tensors (l2s_train_bind; bind the BatchNorm running
 * statistics and the other buffers as well, grad_dev = NULL).  Needs l2s_set_option("refresh_map", 1) before l2s_model_finalize: finalize
 * then records, for every blob float that copies a checkpoint element verbatim, where it comes from; BatchNorm folds and bias sums are
 * recomputed by small kernels; the phase-merged step weights (fp64 products) are marked stale and l2s_decode_steps / l2s_inference use
 * the literal step until the next l2s_model_finalize.  Replaces the host re-pack (~190 ms) by ~1 ms of device work. */
int l2s_train_refresh_weights(l2s_model* m, void* stream);

/* Post-net forward with a tape (decoder.py:143-156, eval-mode BatchNorm statistics) and its backward:
 * mel dev (B,S,80) -> mel_post dev (B,80,S);  dmel_post dev (B,80,S) -> dmel dev (B,S,80) is ACCUMULATED into.
 * drop: NULL (no dropout) or the five dropout multipliers (0 or 1/(1-p), p = 0.5; decoder.py:152,154) channel-last and back to back:
 * layers 0..3 (B*S,512) each at offset l*B*S*512, layer 4 (B*S,80) at offset 4*B*S*512 - explicit inputs, like the Gumbel noise. */
int64_t l2s_train_postnet_tape_floats(int B, int S);
int64_t l2s_train_postnet_ws_bytes(int B, int S);
int l2s_train_postnet_fwd(l2s_model* m, const float* mel, int B, int S, float* tape, float* mel_post, const float* drop, void* stream);
int l2s_train_postnet_bwd(l2s_model* m, const float* mel, const float* dmel_post, int B, int S, float* tape, float* dmel, const float* drop,
                          void* ws, int64_t ws_bytes, void* stream);

/* Stage 2: the autoregressive loop with a tape and its back-propagation through time (decoder.py:353-375; the literal 6-phase
 * step, eval-mode statistics, no dropout).  `state` is the buffer of l2s_decoder_prologue.  Forward: mel dev (B,S,80), stop dev (B,S),
 * attn_logits dev (B,S,T) (also read by the backward).  Backward: dmel dev (B,S,80) = total gradient of the pre-postnet frames,
 * dstop dev (B,S); wbuf = l2s_train_steps_weights_floats() floats filled by l2s_train_steps_pack_weights (transposed step weights packed on
 * the device from the bound canonical parameters - repack after every optimizer step).  Outputs: parameter gradients into the bound
 * slots, dk / dv dev (B,T,512), dckey / dcval dev (B,min_T,256), dh_init dev (2,B,512), de_c dev (B,512).
 * Train-mode dropout sites of the loop as explicit multiplier inputs (0 or 1/(1-p); NULL = site off), the same tensors for fwd and bwd:
 * drop_prenet dev (S,B,256) after the first prenet PSine (p 0.2, decoder.py:308); drop_attn dev (S,B,T) on the attention logits (p 0.1,
 * :363 - the returned attn_logits are the dropped ones, as in the reference); drop_rnn dev (S,B,512) on h0 as input of LSTM layer 1
 * (p 0.1, nn.LSTM(dropout=0.1), :312). */
int64_t l2s_train_steps_tape_floats(int B, int S);
int64_t l2s_train_steps_weights_floats(void);
int64_t l2s_train_steps_ws_bytes(int B, int S);
int l2s_train_steps_pack_weights(l2s_model* m, float* wbuf, void* stream);
int l2s_train_steps_fwd(l2s_model* m, float* state, int B, int T, int S, const float* teacher, const uint8_t* teacher_mask,
                        const uint8_t* teacher_mask_dev, float* tape, float* mel, float* stop, float* attn_logits, const float* drop_prenet,
                        const float* drop_attn, const float* drop_rnn, void* ws, int64_t ws_bytes, void* stream);
int l2s_train_steps_bwd(l2s_model* m, float* state, int B, int T, int S, const uint8_t* teacher_mask, float* tape, const float* attn_logits,
                        const float* dmel, const float* dstop, float* wbuf, float* dk, float* dv, float* dckey, float* dcval, float* dh_init,
                        float* de_c, const float* drop_prenet, const float* drop_attn, const float* drop_rnn, void* ws, int64_t ws_bytes,
                        void* stream);

/* Stage 3: the decoder prologue with a tape (decoder.py:321-351 / 383-410) and its backward down to the visual features.
 * Forward = l2s_decoder_prologue (same `state` buffer, same arguments) plus the tape.  Backward: the gradients of the state the loop
 * consumed (the outputs of l2s_train_steps_bwd; dcontent_dis dev (B*min_T,501) = gradient of the content distribution, may be NULL)
 * -> every prologue parameter gradient into the bound slots and dvis dev (B,T,1024). */
int64_t l2s_train_prologue_tape_floats(int B, int T);
int64_t l2s_train_prologue_ws_bytes(int B, int T);
int l2s_train_prologue_fwd(l2s_model* m, const float* vis, const float* emb, const float* gumbel, int B, int T, float* state, float* content_dis,
                           float* tape, void* ws, int64_t ws_bytes, void* stream);
int l2s_train_prologue_bwd(l2s_model* m, const float* vis, const float* emb, int B, int T, float* state, float* tape, float* wbuf, const float* dk,
                           const float* dv, const float* dckey, const float* dcval, const float* dh_init, const float* de_c, const float* dcontent_dis,
                           float* dvis, void* ws, int64_t ws_bytes, void* stream);

/* Visual encoder with a tape (video.py:76-87, shufflenetv2.py:42-152) and its backward.  Forward = l2s_encoder_fwd (same outputs:
 * vis dev (B,T,1024) and/or feat dev (B,T,768)) plus the tape.  Backward: dfeat = gradient wrt the normalised features, row stride
 * ld_dfeat floats (pass the dvis of l2s_train_prologue_bwd with ld_dfeat = 1024) -> every encoder parameter gradient into the bound
 * slots (the reference computes no gradient wrt the video). */
int64_t l2s_train_encoder_tape_floats(int B, int T, int H);
int64_t l2s_train_encoder_ws_bytes(int B, int T, int H);
int l2s_train_encoder_fwd(l2s_model* m, const float* video, int B, int T, int H, int W, const float* emb, float* vis, float* feat, float* tape, void* stream);
int l2s_train_encoder_bwd(l2s_model* m, const float* video, int B, int T, int H, int W, const float* dfeat, int ld_dfeat, float* tape, void* ws, int64_t ws_bytes,
                          void* stream);

/* ---- training with per-clip video lengths: the training step of a zero-padded batch, forward and backward --------------------------------------
 * l2s_train_<stage>_masked_fwd / _masked_bwd, stage = encoder, prologue, steps (the word order keeps the names l2s_train_*_fwd_masked free: their
 * ABSENCE is what tests/test_masked_lengths_host.py has pinned since the forward-only masked family).
 * The masked forms of the three stages that see the video take their unmasked signature plus `video_lengths`, the HOST array of B int32 of the
 * masked family above ("per-clip video lengths": clips ZERO-padded to T, len_b in [7, T] or an error that names the row, before anything is
 * launched).  Every call carries the lengths to the device itself (csrc/host_table.h: kernel arguments on `stream`, no allocation, no
 * synchronisation; the array may be freed when the call returns) into its TAPE: size the tapes with the *_tape_floats_masked sizers and the
 * workspaces of the encoder and the prologue with *_ws_bytes_masked (the loop keeps l2s_train_steps_ws_bytes).  l2s_train_postnet_* and
 * l2s_loss do not depend on video lengths and are unchanged: the loop runs S steps for every clip, the loss covers padded target frames, as in the
 * reference, and the KLD term keeps its mean over all B * min_T(T) rows (rows of unused slots are zeros and add nothing to the sum).  The forms that
 * honour the MEL lengths as well - l2s_loss_lengths, l2s_train_postnet_masked_* - follow this section.
 * Forward.  Row b of mel, stop and the attention logits - so of mel_post - is what the unmasked training forward gives clip b ALONE at B = 1,
 * T = len_b with the same teacher frames, dropout multipliers and its first m_b = l2s_min_T(len_b) Gumbel rows.  Attention logits at t >= len_b
 * are -INFINITY; content_dis rows of slots >= m_b and the 768 feature columns of vis / feat rows t >= len_b are exact zeros (the speaker
 * columns of vis are the clip's own on every row).
 * Backward.  Every parameter gradient is the sum over the clips of the gradient the unmasked backward computes for that clip alone, fed the same
 * upstream-gradient rows.  dvis rows t >= len_b, dk / dv rows t >= len_b and dckey / dcval of slots >= m_b are exact zeros; the -INFINITY logits
 * give no NaN.  Same bits run to run.  With every len_b = T every output, tape and gradient has the bits of the unmasked entry points.
 * Never read, whatever they hold: drop_attn at columns t >= len_b, rows t >= len_b of dfeat (l2s_train_encoder_masked_bwd), Gumbel rows >= m_b
 * of a clip, dcontent_dis rows of slots >= m_b, and K / V rows t >= len_b of the state.
 * How.  The front-end runs on the padded batch (its temporal zero padding is what makes a padded clip's real frames see what a solo clip sees);
 * the real frames of its pooled map are gathered into a compact list and the trunk runs at sum(len_b) frames, forward and backward; the
 * recurrence of the prologue keeps its T uniform launches with the capture / reset row kernels of the masked inference prologue laid over them
 * and their adjoints over its backward; the attention blocks and their backward run every row over its own frames and slots.
 * Refused by name: batch_stats = 1 (l2s_train_set_bn) - the masked calls run on running statistics; a batch-statistics mode that leaves pad
 * positions out of every BatchNorm does not exist yet, and one that counts them is not offered - and option "train_bf16".  No grouped or
 * ragged training forms. */
int64_t l2s_train_encoder_tape_floats_masked(int B, int T, int H);
int64_t l2s_train_encoder_ws_bytes_masked(int B, int T, int H);
int64_t l2s_train_prologue_tape_floats_masked(int B, int T);
int64_t l2s_train_prologue_ws_bytes_masked(int B, int T);
int64_t l2s_train_steps_tape_floats_masked(int B, int S);
int l2s_train_encoder_masked_fwd(l2s_model* m, const float* video, int B, int T, int H, int W, const float* emb, float* vis, float* feat, float* tape, void* stream,
                                 const int32_t* video_lengths);
int l2s_train_encoder_masked_bwd(l2s_model* m, const float* video, int B, int T, int H, int W, const float* dfeat, int ld_dfeat, float* tape, void* ws,
                                 int64_t ws_bytes, void* stream, const int32_t* video_lengths);
int l2s_train_prologue_masked_fwd(l2s_model* m, const float* vis, const float* emb, const float* gumbel, int B, int T, float* state, float* content_dis,
                                  float* tape, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths);
int l2s_train_prologue_masked_bwd(l2s_model* m, const float* vis, const float* emb, int B, int T, float* state, float* tape, float* wbuf, const float* dk,
                                  const float* dv, const float* dckey, const float* dcval, const float* dh_init, const float* de_c,
                                  const float* dcontent_dis, float* dvis, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths);
int l2s_train_steps_masked_fwd(l2s_model* m, float* state, int B, int T, int S, const float* teacher, const uint8_t* teacher_mask,
                               const uint8_t* teacher_mask_dev, float* tape, float* mel, float* stop, float* attn_logits, const float* drop_prenet,
                               const float* drop_attn, const float* drop_rnn, void* ws, int64_t ws_bytes, void* stream, const int32_t* video_lengths);
int l2s_train_steps_masked_bwd(l2s_model* m, float* state, int B, int T, int S, const uint8_t* teacher_mask, float* tape, const float* attn_logits,
                               const float* dmel, const float* dstop, float* wbuf, float* dk, float* dv, float* dckey, float* dcval, float* dh_init,
                               float* de_c, const float* drop_prenet, const float* drop_attn, const float* drop_rnn, void* ws, int64_t ws_bytes,
                               void* stream, const int32_t* video_lengths);

/* ---- training with per-clip mel lengths: the loss and the post-net of a batch whose TARGETS are padded to S ---------------------------------------------
 * The other half of the padding above.  mel_lengths: a HOST array of B int32, S_b in [1, S] (the collates' melspec_lengths; targets padded with finite
 * values, the gate target 1 from frame S_b - 1 on); video_lengths as above, or NULL where the model did not honour them (every clip then owns all
 * m = R / B content rows).  Each call carries its table to the device itself (csrc/host_table.h: kernel arguments on `stream`, no allocation, no
 * synchronisation, no copy from pageable memory; the arrays may be freed when the call returns) - l2s_loss_lengths into its scratch, the post-net calls
 * into their tape.
 * l2s_loss_lengths: l2s_loss's arguments, then the two length arrays, T (the padded frame count video_lengths refers to; ignored with NULL) and per_clip.
 *   The batch loss is (1/B) sum_b of the loss of clip b ALONE, each term over the clip's own extent: the two mel MSEs over 80 * S_b, BCE over S_b, KLD over
 *   the clip's own m_b = l2s_min_T(len_b) rows (rows b * m .. b * m + m_b of content_dis).  losses5 as l2s_loss; per_clip dev (B,4) or NULL: each clip's own
 *   four terms.  Gradients: dmel[b,:,s] = 2 d / (B * 80 * S_b), dmel_post 10 x that, dstop = (sigmoid(x) - y) / (B * S_b), ddis of a used row scaled by
 *   1 / (B * m_b); every gradient element at s >= S_b and every ddis row >= m_b of a clip is an EXACT ZERO, written by the same pass (no pre-clearing; l2s_loss
 *   gives a zero row of content_dis the gradient log(1e-20), this call does not).  Nothing at a pad position of mel, mel_post, stop, the targets, or a
 *   content row >= m_b is read.  Two-stage fp64 like l2s_loss - per-(clip, term) partials, then one block that divides per clip and averages over B: the same
 *   bits run to run; two launches plus the table's.  With every S_b = S and every m_b = m the call runs l2s_loss's own launches: its bits, terms and gradients
 *   (the length-aware pass then only fills per_clip).
 *   l2s_loss_lengths_check: the pure host validator the call runs first - B in [1, 96], every S_b in [1, S] ("mel_lengths[1] = 9 is outside [1, S = 8]"), a
 *   null table, and video_lengths (when given) as the masked family checks them; nothing is launched on an error.
 *   scratch: l2s_train_scratch_bytes_lengths(B) (l2s_loss's scratch, the partials, the device table); -1 outside B in [1, 96].
 * l2s_train_postnet_masked_fwd / _masked_bwd: the unmasked signatures plus mel_lengths.  (Word order as above: the *_fwd_masked names stay free.)
 *   Forward: `mel` is NOT const - rows s >= S_b, which the loop decoded past the clip's end, are zeroed in place - and the rows s >= S_b of every layer's
 *   input (mel, x_0 .. x_3) are zeros, so rows < S_b of mel_post are what the unmasked post-net gives the clip alone at S = S_b; mel_post[b,:,s >= S_b] is
 *   exact zeros.  Backward: the adjoint of the same zeroing: pad positions of dmel_post count as zeros whatever they hold, pad rows of every input gradient
 *   are zeroed after each dx, so nothing flows from a real row into a pad row, and pad rows add exact zeros to the weight, bias, BatchNorm-affine and PSine
 *   gradients; pad rows of dmel receive an added exact zero.  Dropout multipliers at pad rows never reach a result (NaN there changes nothing).  With every
 *   S_b = S: the bits of the unmasked calls (the same launches; the row kernels find nothing to zero).  About ten short launches more per step.
 *   Tape: l2s_train_postnet_tape_floats_masked (the unmasked tape plus the table); workspace: l2s_train_postnet_ws_bytes_masked (= the unmasked size).
 * The loop is unchanged - clip b still runs S steps; with exact-zero dmel / dstop at its pad steps, BPTT adds exact zeros for them.  Teacher frames and the
 * loop's dropout multipliers at pad steps must be finite: the loop reads them.
 * Refused by name, before any launch: S_b outside [1, S] or a null table (the clip is named), batch_stats = 1 (the post-net's BatchNorms would have to take
 * their statistics over real rows only: not built) and option "train_bf16". */
int l2s_loss_lengths_check(const int32_t* mel_lengths, const int32_t* video_lengths, int B, int S, int T);
int64_t l2s_train_scratch_bytes_lengths(int B);
int l2s_loss_lengths(const float* mel, const float* mel_post, const float* mel_target, const float* stop, const float* gate_target,
                     const float* content_dis, int B, int S, int R, float* losses5, float* dmel, float* dmel_post, float* dstop, float* ddis,
                     void* scratch, void* stream, const int32_t* mel_lengths, const int32_t* video_lengths, int T, float* per_clip);
int64_t l2s_train_postnet_tape_floats_masked(int B, int S);
int64_t l2s_train_postnet_ws_bytes_masked(int B, int S);
int l2s_train_postnet_masked_fwd(l2s_model* m, float* mel, int B, int S, float* tape, float* mel_post, const float* drop, void* stream,
                                 const int32_t* mel_lengths);
int l2s_train_postnet_masked_bwd(l2s_model* m, const float* mel, const float* dmel_post, int B, int S, float* tape, float* dmel, const float* drop,
                                 void* ws, int64_t ws_bytes, void* stream, const int32_t* mel_lengths);

/* ---- run-time options ------------------------------------------------------------------------------------------------------------
 * l2s_set_option changes the PROCESS DEFAULTS: what l2s_model_create copies into a new model.  l2s_model_set_option changes one model.
 * Launch sequences only ever read their own model's copy, so a thread that flips a switch cannot disturb batches other threads have in
 * flight on other models.  Several host threads may also drive ONE model at once (lip2speech_amd.parallel.InflightPool: chains in flight on
 * one weight blob): the blob is read-only, every workspace is its caller's, the per-model side stream / events / graph cache behind
 * "use_graph" are serialised by a per-model mutex, and the l2s_profile_* accumulators are guarded - only changing an option of a model WHILE
 * other threads run batches on it is the caller's race.  An unknown name is an error.  The options of the product library choose WHAT is
 * computed (precision leg, semantics) or a documented mode; the switches that only choose between block forms of the same arithmetic
 * (measured and rejected forms, kept for A/B timing) exist in the diagnostic build alone: include/l2s_diag.h.
 *   "persist_decode"    (4)  the free-running decode loop (decoder.py:412-435) of a single-batch call with at most this many clips - up to 4, clips of
 *                            <= 32 frames (demo.py runs one clip, BASELINE config 1 two) - as ONE persistent launch of 128 resident workgroups per clip
 *                            that keep the step weights in registers and exchange h / c / q / prenet as tagged 8-byte granules (pdecode.hip): 7.7 instead
 *                            of 20.4 us per step at one clip, 8.2 at two; three or four clips run as two such launches one after the other.  Another
 *                            order of the same fp32 sums (within 5e-4 of the launch path, < 1e-3 of the reference).  The form is only taken where
 *                            l2s_persist_available() says every workgroup can be resident; a launch that makes no progress for 2 s gives up,
 *                            overwrites mel / stop / attention with NaN and counts in l2s_persist_timeouts(); the NEXT persistent-eligible call on that
 *                            device fails once with that error, later ones take the launch path until the option is set to a positive value again
 *                            (which re-arms the device).  0 = always four launches per step; l2s_*_multi never uses it
 *   "persist_frames"    (32) the longest clip, in frames, whose calls take the persistent forms above.  At the default only clips of <= 32 frames do,
 *                            exactly as before the option existed.  Above 32 (the built maximum is 80: GRID's 75-frame clips, AVSpeech's 26-50) clips
 *                            of 33 .. min(value, 80) frames take the long-clip forms of the same loop: two key frames per thread in registers, the keys
 *                            of frames 64 .. 79 in LDS, a soft-max lane carrying two frames (256 VGPRs + 216 AGPRs, no scratch; LDS <= 134 KB), and
 *                            for one or two clips the persistent BiLSTM of the prologue as well.  Clips of <= 32 frames launch the same kernels
 *                            whatever the value; masked, teacher-forced, grouped and "use_graph" calls and clips of more than 80 frames keep the launch
 *                            path; "early_stop" composes.  Same bounds as the short forms (5e-4 of the launch path, 1e-3 of the reference); where
 *                            a long form does not fit one workgroup per compute unit the long envelope alone is off on that device.  Measured
 *                            against the launch path, same call, S = 300 (profiles/persist_long_times.txt): one clip of 75 frames 9.6 -> 3.8 ms,
 *                            two 9.5 -> 4.0, four (two launches in sequence) 10.2 -> 7.5; 50 frames: 8.5 -> 3.5, 8.3 -> 3.7, 8.7 -> 6.8
 *   "persist_masked"    (0)  > 0: the *_masked entry points take the persistent forms above as well, where the call is otherwise inside their envelope:
 *                            free-running (l2s_inference_masked, l2s_decode_steps_masked without teacher frames, l2s_decoder_prologue_masked), not
 *                            "use_graph", B <= min("persist_decode", 4), PADDED T <= max(32, min("persist_frames", 80)), l2s_persist_available().  A
 *                            clip's workgroups read its length from the device length table and run the loop of a len_b-frame clip (the padded T is
 *                            only the row pitch of keys, values and attention); every launch of one or two clips takes the form and the LDS of ITS
 *                            longest clip, so two short clips under long padding take the short form.  The prologue's BiLSTM runs len_b steps per
 *                            (direction, clip) at B <= 2; at B = 3, 4 the prologue keeps the launch route, as for unmasked calls.  Attention columns
 *                            t >= len_b are exactly 0 (-INFINITY as logits), as on the launch route.  Row b is within 5e-4 of the masked launch route
 *                            and 1e-3 of clip b alone on the reference; all lengths = T gives the bits of the unmasked persistent call, and a clip's
 *                            row has the same bits beside another partner or under another padding when the clip count and the form are the same
 *                            (DESIGN.md section 8).  "early_stop" composes.  Teacher-forced calls (l2s_forward_eval_masked, teacher frames) and
 *                            calls outside the envelope keep the launch route, bit for bit.  0 = masked calls never take the persistent forms,
 *                            exactly as before the option existed.  Not yet timed on an MI355X (tools/persist_masked/time_persist_masked.py writes
 *                            profiles/persist_masked_times.txt, B = 3, 4 - two launches in sequence - included); the expectation is the unmasked
 *                            figures under "persist_frames" above: the same loop over fewer frames
 *   "use_graph"         (0)  replay the decode loop from a captured hipGraph (BASELINE config 4's streaming decoder; slower than plain launches
 *                            on this runtime at every size measured, so off by default)
 *   "fold_step_weights" (1)  4-launch step with pre-multiplied prenet1*fc_out and attention_proj hoisted onto the values; 0 = the literal 6-phase
 *                            step of decoder.py:412-429 (what a model runs after l2s_train_refresh_weights until its merged weights are rebuilt)
 *   "refresh_map"       (0)  l2s_model_finalize also builds the map l2s_train_refresh_weights needs (training)
 *   "infer_bf16"        (0)  the bf16 leg of the INFERENCE / evaluate entry points: the front-end conv on one bf16 plane, GEMMs / Conv1d stacks of
 *                            encoder, prologue, post-net and voice tower with bf16 operands and fp32 accumulation; the decode loop, the BiLSTM, the
 *                            fused ShuffleNet units and every activation in HBM stay fp32.  Outside the 1e-3 fp32 gate by construction
 *   "train_bf16"        (0)  TRAINING entry points (encoder, prologue, post-net; forward and backward): GEMMs / Conv1d stacks round their operands to
 *                            bf16 (RNE) on the way into LDS, fp32 accumulation and results; the recurrent loop, the Conv3d front-end, BatchNorm
 *                            statistics, master weights and optimizer stay fp32
 *   "gemm_x3"           (1)  inference GEMMs / Conv1d stacks on the bf16 matrix cores through the EXACT three-way split (x = hi + mid + lo, six bf16
 *                            MFMAs per K step of 16 instead of eight f32 MFMAs of K = 2) where the shapes are eligible; 0 = the f32 MFMA kernel
 *   "frontend_x3"       (3)  the inference front-end conv (Conv3d 5x7x7 + BN + PReLU + MaxPool) on the same split-bf16 path: 3 = two consecutive
 *                            output frames per block with the next slab's staging interleaved between the MFMAs, 2 = the same with a staging phase of its
 *                            own (same bits), 1 = one frame per block, 0 = the f32 MFMA kernel
 *   "trunk_x3"          (1)  the fused ShuffleNet units' pointwise convs on the split-bf16 path; 0 = f32 MFMA
 *   "lstm_x3"           (4)  the decode step's two LSTM launches on the split-bf16 path (1 / 2 / 3: four-wave / eight-wave / half-CU block forms of the
 *                            same arithmetic, same bits - 3 picks by l2s_set_thread_chains; 4 = as 3, with the K = 1024 launches as one 64 x 64 block
 *                            per CU whose column halves share one activation panel); 0 = f32 MFMAs (other bits, rounding-level)
 *   "early_stop"        (0)  free-running inference (l2s_inference, l2s_inference_multi, l2s_decode_steps without teacher frames) ends the decode loop once
 *                            every clip of the call has stopped, instead of always running S steps as the reference does (decoder.py:412-435).  With
 *                            len_b = the clip's output_lengths entry, E_b = min(S, len_b + 10) and E = max E_b over the call's rows (all G x B of a group):
 *                            the post-net is five Conv1d layers of kernel 5, so frame j < len_b of mel_post reads decoded frames up to len_b + 9 only, and
 *                            decoding E_b steps gives every kept frame the inputs of the S-step pass.  On:
 *                              - lengths are exactly the option-off lengths; shapes stay (B,80,S) / (B,S,T);
 *                              - mel_post[b][:][j] and attn[b][j][:] for j < len_b are the S-step values (same bits on the launch-per-phase route);
 *                              - for j >= len_b - what every caller drops - both are exactly 0: the reference's output masked by its own lengths;
 *                              - l2s_decode_steps' staged mel / stop / attention: steps < E_b as with the option off, steps >= E exactly 0, steps in
 *                                [E_b, E) computed on the launch-per-phase route (the batch runs until its last clip ends) and 0 on the persistent route
 *                                (each clip leaves on its own); the buffers are zero-filled on the stream first, nothing stays unwritten;
 *                              - a call with a clip that never stops (len_b = S) runs to S: the option-off call plus the masking.
 *                            The decision is made on the device - the host enqueues all S steps without synchronising; the step kernels past the end
 *                            return at their top (launch route), the persistent loop's workgroups leave their loop.  The post-net still runs over all
 *                            S frames (of zeros past E).  Ignored by l2s_forward_eval(_multi), teacher-forced l2s_decode_steps and the training entry
 *                            points (their S comes from the target).  With "use_graph" the call takes the plain launch route (a replayed graph carries
 *                            no control block of the call); the diagnostic post-net overlap ("overlap_postnet") likewise takes the plain route */
int l2s_set_option(const char* name, int value);
int l2s_model_set_option(l2s_model* m, const char* name, int value);
/* The persistent forms (option "persist_decode") spin on other workgroups and need all of them resident at once.  l2s_persist_available: 1 where that
 * holds on the current device - 256 compute units, no compute-unit mask in the environment (HSA_CU_MASK / ROC_GLOBAL_CU_MASK), one workgroup of every
 * persistent kernel fits a compute unit (occupancy query), and no persistent launch on this device has timed out since it was last armed - else 0: calls
 * inside the envelope then take the launch-per-phase path.  l2s_persist_timeouts: how many persistent launches of this process gave up (2 s without
 * progress) and had their outputs overwritten with NaN; read from pinned host memory, no synchronize - meaningful after the host has synchronized with
 * the stream.  The library itself reports a time-out through the next persistent-eligible call on that device (it fails once; l2s_last_error). */
int l2s_persist_available(void);
int l2s_persist_timeouts(void);
/* How many launch chains the CALLER keeps in flight on the device, for the calling host thread (default 1): a scheduling hint, never arithmetic.  With
 * n >= 2 the step kernels of this thread's calls take blocks of half a compute unit, so that kernels of the other chains run beside them on the same
 * CUs - 33.6 -> 27-28 us per decode step for the chip at 256 rows with three chains; with n = 1 they keep the blocks that fill a CU, which are 3-4 %
 * faster when the chain has the chip to itself.  lip2speech_amd.parallel.InflightPool sets it in its worker threads. */
int l2s_set_thread_chains(int n);
/* per-kernel timing: when enabled every launch is bracketed by HIP events on its stream; read back with
 * l2s_profile_get (which synchronises the events it reads).  Off by default. */
int l2s_profile_enable(int on);
int l2s_profile_reset(void);
int l2s_profile_count(void);
int l2s_profile_get(int idx, const char** name, int64_t* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* L2S_H */
