// Internal launch interface between the host side of libbbocr (ctx.h and the .cpp translation units) and the HIP kernels.  Not public.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

// ------------------------------------------------------------------ implicit-GEMM convolution (conv_mfma.hip)
struct ConvArgs {
    const uint16_t* in0;   // bf16 NHWC source 0
    const uint16_t* in1;   // bf16 NHWC source 1 (virtual channel concat after source 0) or null
    const uint16_t* wpk;   // packed bf16 weights, see pack_conv_weights()
    const float* bias;     // fp32 [Cout_pad] (BN folded), natural cout order
    void* out;             // bf16 or fp32 NHWC
    int C0, C1;            // channels taken from each source (multiples of 32)
    int in0_cs, in1_cs;    // pixel strides (elements) of the sources
    int N, H, W, OH, OW;
    int KH, KW, pad_h, pad_w, dil;
    int TH, TW, tiles_x, tiles_y, ntiles_n;
    int PH, PW, NP;        // activation patch (TH+(KH-1)dil) x (TW+(KW-1)dil), NP = roundup16(PH*PW)
    int relu_in0, relu_in1, relu_out, out_f32;
    int out_cs, cout_store;  // output pixel stride (elements), couts actually stored (multiple of 16)
    int nchunks, ntaps;
    // fused max-pool in the epilogue: 0 none, 1 = MaxPool2d(2,2), 2 = MaxPool2d((2,1),(2,1)); bf16 output [N,OH/2,OW(/2),pool_cs]
    int pool_mode, pool_relu, store_full, pool_cs;
    void* pool_out;
    // aux_w (see aux_b) sits apart from aux_b on purpose: argument offsets decide how hipcc merges the kernels' argument loads, and this
    // order compiles every conv kernel with the register and spill counts they were measured with
    const uint16_t* aux_w;
    const float* tail;     // non-null: fuse the CRAFT classifier tail (two 1x1 convs on 16 channels) into the epilogue (BN=64 config,
                           // cout_store 16): {b1[16], w2[32], b2[2]}; tail_frag: W1 as a bf16 MFMA A fragment [64 lanes][8]
    const uint16_t* tail_frag;
    // post_w: a 1x1 conv 64 -> 64 (no bias, no ReLU) applied to the finished 64 output channels in the epilogue, packed by
    // pack_post1x1_weights; only the product is stored (CRAFT: z = W_y u3b behind upconv3's 3x3, launch_conv declines other shapes)
    const uint16_t* post_w;
    int sub;               // > 1: dilated 3x3 run as sub*sub plain convs on the phase sub-lattices (set by launch_conv)
    int stack;             // sub > 1: rows of one phase image; the sub*sub images of a page are stacked along y, one zero row apart
    const void* zero;      // >= 16 zero bytes in device memory (source of padding pixels for the LDS-DMA staged variant)
    // non-null: add the 2x bilinear up-sampling (align_corners=False) of this bf16 NHWC tensor [N, up_H/2, up_W/2, up_cs] to the
    // accumulators before bias/ReLU -- conv1x1(cat[up(y), s]) == up(conv1x1_y(y)) + conv1x1_s(s): the U-net 1x1 layers never
    // materialise up(y).  up_H/up_W: size of the (full-resolution) output image; plain store path only.
    const uint16_t* addup;
    int up_H, up_W, up_cs;
    // non-null: CRAFT conv1_2 with conv1_1 fused in -- in0 is the uint8 RGB batch [N, rgb_H, rgb_W, 3] on the H x W canvas,
    // c11_w the conv1_1 weights packed by pack_conv1_1_weights_fused, c11_b its 64 biases (C0 stays 64)
    const uint16_t* c11_w;
    const float* c11_b;
    int rgb_H, rgb_W;
    // conv3x3_up4_kernel (CRAFT upconv4 as ONE launch): in0 = the skip tensor s1 [N,H,W,128], addup/up_* = z = W_y y at half resolution,
    // aux_w / aux_b = the packed 1x1 weights (64 couts x 128 cin, BN = 64 plan) and bias of upconv4.conv.0; wpk / bias = upconv4.conv.3
    const float* aux_b;
    float acc_scale;       // accumulators are multiplied by this before the bias (set from ConvPlan::acc_scale by launch_conv; 1 unless
                           // the packed weights carry a power-of-two scale, see the split-fp16 plans)
    int lean;              // conv3x3_dma_kernel: which epilogue (set by its launcher: 0 shared, 1 plain lean, 3 pooled lean)
    int split_off;         // > 0 (fp16 element type only): every stored value v goes out as the pair hi = fp16(v) at its channel and
                           // lo = fp16(v - hi) at channel + split_off -- the [hi | lo] activation layout of the exact recogniser mode
    int add_same;          // 1: `addup` is a tensor at the OUTPUT's own resolution [N, H, W, up_cs], added pixel by pixel before bias/ReLU (no
                           // up-sampling): out = ReLU(z + W_s s + b), the second launch of detector.cpp::craft_fc_stage.  Read by the launcher
                           // only (it picks the kernel's epilogue); last, so that no other member moves
};

struct ConvPlan {      // host-side description of one packed conv layer
    int Cin = 0, Cout = 0;     // logical sizes
    int Cin_pad = 0, Cout_pad = 0;
    int KH = 1, KW = 1, pad_h = 0, pad_w = 0, dil = 1;
    int BN = 64;       // cout tile of the launch config chosen for this layer (64/128/256)
    int el = 0;        // element type of the packed weights and of the activations this layer reads / writes: 0 bf16, 1 fp16
    float acc_scale = 1.f;   // 2^-s when the packed weights are w * 2^s (exact; split-fp16 plans keep w_lo out of fp16's subnormals)
    int split = 0;     // 1: split-fp16 plan (weights.cpp::upload_split_plan): Cin counts the three blocks [a_hi | a_lo | a_hi]
    uint16_t* d_w = nullptr;   // device packed weights
    float* d_b = nullptr;      // device bias [Cout_pad]
};

// Which kernel launch_conv took: one id per terminal of the dispatch (conv_mfma.hip, launch_conv_el and the launchers under it).  Host side
// only -- it is NOT part of ConvArgs, whose layout the kernels' register counts depend on.  include/bbocr.h mirrors the ids (BBOCR_ROUTE_*)
// and the struct (bbocr_conv_route: the same ints in the same order, pinned by static_asserts in abi_ops.cpp).
enum ConvRouteId : int {
    CONV_ROUTE_NONE = 0,            // nothing launched (a refusal)
    // conv_mfma_kernel, the register-staged generic kernel: <EL, 4, 1, 4, PITER> (64 couts per tile) / <EL, 2, 2, 8, PITER> (128)
    CONV_ROUTE_GEN64_P4, CONV_ROUTE_GEN64_P8, CONV_ROUTE_GEN64_P16, CONV_ROUTE_GEN128_P4, CONV_ROUTE_GEN128_P8, CONV_ROUTE_GEN128_P16,
    // conv3x3_dma_kernel, 64 couts per tile: conv1_1 fused in (FUSE1) / 1x1 behind the layer (EPI 1)
    CONV_ROUTE_DMA64_FUSE1, CONV_ROUTE_DMA64_POSTW,
    // conv3x3_resw_kernel: <EL, 1, true, 4, true> (64 couts, pooled) / <EL, 1, true> (one chunk) / <EL, 2, false> (two chunks)
    CONV_ROUTE_RESW_POOL64, CONV_ROUTE_RESW_1CH, CONV_ROUTE_RESW_2CH,
    // conv3x3_dma_kernel, 64 couts: 324-slot patch with two / four cout fragments per wave, 384 slots, 448 slots (NPB 7)
    CONV_ROUTE_DMA64_324_NF2, CONV_ROUTE_DMA64_324, CONV_ROUTE_DMA64_384, CONV_ROUTE_DMA64_448,
    // conv3x3_dma_kernel, 128 couts: 384 slots behind a 4-deep weight ring, 448 slots behind a 3-deep one
    CONV_ROUTE_DMA128_384, CONV_ROUTE_DMA128_448,
    // conv3x3_dma_kernel with KS = 2 (2x2, padding 0)
    CONV_ROUTE_DMA2X2_64, CONV_ROUTE_DMA2X2_128,
    // conv1x1_dma_kernel: by couts per tile without an addend in the epilogue; with one (ADDUP: ConvRoute::addup says which, any tile width: see ConvRoute::wn)
    CONV_ROUTE_DMA1X1_64, CONV_ROUTE_DMA1X1_128, CONV_ROUTE_DMA1X1_256, CONV_ROUTE_DMA1X1_ADDUP,
    CONV_ROUTE_COUNT
};
struct ConvRoute {
    int id;                                                     // ConvRouteId
    int status;                                                 // hipError_t the launcher returned (0: launched, or would have been)
    // template numbers of the terminal (0 where the family has none)
    int el, wm, wn, mf;
    int piter;                                                  // conv_mfma_kernel
    int npb, ring, nps, fuse1, nf, epi, ks;                     // conv3x3_dma_kernel
    int addup;                                                  // conv1x1_dma_kernel (its RING is `ring`): 1 the up-sampling epilogue, 2 the
                                                                // same-resolution addend (ConvArgs::add_same); both under CONV_ROUTE_DMA1X1_ADDUP
    int resw;                                                   // conv3x3_resw_kernel: 1 <1, true, 4, true>, 2 <1, true>, 3 <2, false>
    // geometry the launchers settled
    int OH, OW, TH, TW, PH, PW, NP, sub, stack, tiles_x, tiles_y, ntiles_n, nchunks, ntaps, lean;
    int grid, threads;                                          // workgroups, threads per workgroup
    int persistent;                                             // > 0: the grid is min(tiles, persistent * compute units); a dry run, which
                                                                // asks no device, reports the tile count as `grid`
    int lds_bytes;                                              // dynamic LDS of the launch
    int tail, split_off;                                        // epilogue switches of ConvArgs that select no kernel but change what is stored
};

int conv_plan_bn(int Cout);   // cout tile (64/128/256) of the launch configuration used for a layer
size_t conv_packed_elems(const ConvPlan& p);
// w: fp32 [Cout][Cin][KH][KW] already BN-folded; out: bf16 bits, layout [ntile][chunk][tap][frag][lane][8]
void pack_conv_weights(const ConvPlan& p, const float* w, uint16_t* out);
// a.zero must be set (device zero page).  route: filled by the terminal the dispatch reaches (id CONV_ROUTE_NONE and the status when it
// refuses the shape).  dry: walk the same dispatch and return at the terminal, before any HIP call -- the status is the one a launch would
// give for a shape refusal; pointers of `a` and `p` are only tested for null then.
hipError_t launch_conv(const ConvPlan& p, ConvArgs a, hipStream_t s, ConvRoute* route = nullptr, bool dry = false);
// upconv4 of CRAFT fused: u4b = relu(conv3x3(relu(up(z) + W_s s1 + b_s)) + b): p1 = the 1x1 plan over s1 (128 -> 64), p3 = the 3x3 plan (64 -> 32).
// a: in0 = s1 (in0_cs = 128), addup = z (up_cs = 64), N/H/W of the full-resolution image, out/out_cs/cout_store of u4b.  Returns
// hipErrorNotSupported when the shapes are not the ones the kernel is built for (the caller then runs the two launches).
hipError_t launch_up4_fused(const ConvPlan& p1, const ConvPlan& p3, ConvArgs a, hipStream_t s);

// ------------------------------------------------------------------ detector front/back (craft_misc.hip)
void pack_post1x1_weights(const float* w /*[64][64] cout x cin*/, uint16_t* out /*[2][4][64][8]*/, int el);
void pack_conv1_1_weights_fused(const float* w /*[64][3][3][3] folded*/, uint16_t* out /*[4][64][8]*/, int el);   // one k-step: taps 2g, 2g+1 per lane group, tap 8 in the pad slots; couts in the conv epilogue's run order
hipError_t launch_maxpool(const uint16_t* in, uint16_t* out, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                          int relu_in, hipStream_t s);
hipError_t launch_gray(const uint8_t* rgb, uint8_t* gray, size_t npix, hipStream_t s);
// cv2 BGR2GRAY of one pixel, channels as given (the formula is stated at gray_kernel, craft_misc.hip); also pages.hip's derived gray plane
__device__ __forceinline__ uint8_t bgr2gray_px(int c0, int c1, int c2) { return (uint8_t)((c2 * 9798 + c1 * 19235 + c0 * 3735 + (1 << 14)) >> 15); }
hipError_t launch_ycc_to_rgb_gray(const uint8_t* ycc, int stride, uint8_t* rgb, uint8_t* gray, size_t npix, hipStream_t s);
// jdcolor.c::ycc_rgb_convert of one pixel (the formulas are stated at ycc_to_rgb_gray_kernel, craft_misc.hip); also thumb.hip's last pass
__device__ __forceinline__ void jpeg_ycc_to_rgb(int y, int cb, int cr, uint8_t* rgb) {
    cb -= 128;
    cr -= 128;
    int r = y + ((91881 * cr + 32768) >> 16);
    int g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    int b = y + ((116130 * cb + 32768) >> 16);
    rgb[0] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    rgb[1] = (uint8_t)(g < 0 ? 0 : (g > 255 ? 255 : g));
    rgb[2] = (uint8_t)(b < 0 ? 0 : (b > 255 ? 255 : b));
}
hipError_t launch_resize_u8(const uint8_t* src, int N, int sh, int sw, int C, uint8_t* dst, int dh, int dw, hipStream_t s);

// ------------------------------------------------------------------ exact detector, element-wise helpers on pair tensors (craft_pair.hip)
// pair tensor = [hi C | lo C] fp16 per pixel, value = hi + lo / 2048 (REC_SPLIT below); C % 8 == 0 everywhere
hipError_t launch_pair_conv1_1(const uint8_t* rgb, int N, int Hi, int Wi, int H, int W, const float* w /*[64][3][3][3] folded*/, const float* b, uint16_t* out,
                               hipStream_t s);
hipError_t launch_pair_relu(const uint16_t* in, uint16_t* out, size_t npix, int C, hipStream_t s);
hipError_t launch_pair_maxpool3x3s1(const uint16_t* in, uint16_t* out, int N, int H, int W, int C, hipStream_t s);
// out = cat([interpolate(y -> H x W, bilinear, align_corners=False), skip]) (yh x yw == H x W: plain concat)
hipError_t launch_pair_upcat(const uint16_t* y, int yh, int yw, int Cy, const uint16_t* skip, int Cs, uint16_t* out, int N, int H, int W, hipStream_t s);
hipError_t launch_pair_cls_tail(const uint16_t* in /*[npix, 16 | 16]*/, const float* w1 /*[16][16]*/, const float* tail /*b1[16] w2[32] b2[2]*/, float* heat,
                                size_t npix, hipStream_t s);

// ------------------------------------------------------------------ box extraction (ccl.hip)
struct CclOut {        // per accepted component, device-written, host-sorted by root
    int root, left, top, right, bottom, area, row_off, img;
};
// label/slot: [N*h*w]; stat: [N*h*w][6]; comps: [cap_comps] and rowext: [cap_rows][2] for the WHOLE batch; counters: [4] = ncomps, nrows, overflow
hipError_t launch_ccl(const float* heat, int N, int h, int w, float low_text, float link_thr, double text_thr, int* label, int* stat,
                      int* slot, CclOut* comps, int* rowext, int* counters, int cap_comps, int cap_rows, hipStream_t s);

// ------------------------------------------------------------------ recogniser (crnn_misc.hip, lstm.hip, ctc.hip)
struct CropDesc {      // one recogniser input, filled on the host
    int img;           // page index in the batch
    int sx0, sy0, sw, sh;   // source rectangle: in the gray page, or (0,0,ww,wh) of the warped crop when warp != 0
    int rw, rh;        // cv2.resize target; rh == 64 unless the box is taller than wide (then rw == 64)
    int fw;            // content width after AlignCollate (<= imgW)
    int imgW;          // padded width (bucket)
    int slot;          // row inside the bucket tensor
    int warp;          // 1: four_point_transform crop, uses Minv
    int warp_off;      // byte offset of the warped crop in the warp scratch
    int a_off;         // byte offset of the stage-A (cv2-resized) crop in the crop scratch
    int lut_off;       // >= 0: contrast LUT (256 bytes) offset, -1: none
    int pad_;          // wide recogniser image: first pooled row (time step) of this crop in the sequence tensors
    int rot;           // rotation_info variant: the stage-A image is np.rot90(resized crop, rot); rw x rh are its dimensions AFTER the rotation
    double Minv[9];    // dst -> src homography (already inverted)
};
struct CropPage {      // a gray page of its own shape (bbocr_readtext_pages): CropDesc::img indexes a device table of these
    long long off;     // byte offset of the page's first pixel from the `gray` pointer of the launch
    long long pitch;   // bytes per row
    int H, W;
};
// stage_mask bit0: gather (warp) + cv2 resize into scratch; bit1: (PIL bicubic) + LUT + normalise + pad into out_bucket
// pages != null: the source of crop d is the page pages[d.img] (its own bounds and pitch) instead of plane d.img of [B][H][W]
hipError_t launch_crops(const uint8_t* gray, int H, int W, const CropDesc* descs_dev, int first, int count, int imgW, int any_warp,
                        int any_tall, uint8_t* wscratch, uint8_t* scratch, uint8_t* hscratch, const uint8_t* luts, uint16_t* out_bucket,
                        int stage_mask, hipStream_t s, int wide_row_stride = 0, int gap = 0, int mode = 0,   // wide_row_stride > 0: ONE image [64][Wt], slot = first column
                        const CropPage* pages = nullptr);
// Recogniser tensor modes (bbocr_config::precision): REC_BF16 / REC_F16 = 16-bit elements; REC_SPLIT = the exact mode: the crop image
// holds CODES (0 = padding zero, 1 + grey level otherwise -- conv0 rebuilds the fp32 input ((g/255 - 0.5)/0.5) exactly), every later
// activation is a pair of fp16 tensors [hi C | lo C] per pixel with value = hi + lo / 2048 (lo scaled so that it stays in fp16's
// normal range), the LSTM reads an fp32 input projection.
enum { REC_BF16 = 0, REC_F16 = 1, REC_SPLIT = 2 };
constexpr float SPLIT_LO_SCALE = 2048.f;
hipError_t launch_crop_hist(const uint8_t* scratch, const CropDesc* descs_dev, int first, int count, unsigned int* hist, hipStream_t s);
hipError_t launch_crnn_conv0(const uint16_t* in, const float* w /*[9][32] tap-major*/, const float* b, uint16_t* out, int n, int W, int mode, hipStream_t s,
                             const uint16_t* afrag = nullptr /*pack_crnn_conv0_mfma: the MFMA form (bf16 / fp16 modes, W % 4 == 0)*/);
void pack_crnn_conv0_mfma(const float* w_tap_major /*[9][32]*/, uint16_t* out /*[2][64][8]*/, int el);
// wide recogniser image (all crops side by side, CropDesc::slot = first column, ::pad_ = first pooled row): clear the separator
// columns of a layer output [H][Wl][C] (shift = log2 horizontal down-scale), and the 3-row mean gathered into the pooled rows
hipError_t launch_crnn_zero_gaps(uint16_t* t, const CropDesc* descs_dev, int first, int count, int H, int Wl, int C, int shift, hipStream_t s);
hipError_t launch_rowmean3_gather(const uint16_t* in, int Wc, int C, const CropDesc* descs_dev, int first, int count, uint16_t* out, int mode,
                                  hipStream_t s);   // C: logical channels
// BiLSTM recurrence: xproj bf16 [n,T,2048] (permuted channels, see lstm8_xproj_channel), out bf16 [n,T,512] (fwd | bwd)
// tiles_dev: int4 per workgroup {first row, sequences (<=16), T, 0}; tensors are pooled over all buckets: [rows, C]
// mode REC_SPLIT: xproj is FP32 [rows, 2048], out is the pair [rows, 512 hi | 512 lo] with the lo half UNSCALED (fp16(h - hi): the linear
// layer behind it is packed with lo scale 1), whh_pk comes from pack_lstm_whh_split and acc_scale is the inverse of its weight scale;
// tiles hold up to lstm_tile_seqs(mode) sequences
hipError_t launch_lstm(const void* xproj, const uint16_t* whh_pk, uint16_t* out, const int* tiles_dev, int ntiles, int mode, float acc_scale,
                       hipStream_t s);
int lstm_tile_seqs(int mode);    // sequences per LSTM workgroup (tile table entries): 16 in every mode as built (REC_SPLIT: 16 * LSTMX_NG, lstm.hip)
size_t lstm_whh_packed_elems();
void pack_lstm_whh8(const float* whh_fwd, const float* whh_bwd, uint16_t* out, int el);
size_t lstm_whh_split_packed_elems();
float pack_lstm_whh_split(const float* whh_fwd, const float* whh_bwd, uint16_t* out);   // -> acc_scale (2^-s)
int lstm8_xproj_channel(int dir, int gate, int unit);
// BiLSTM input projection of the 16-bit modes (seq_proj.hip): x [rows_pad, 256] -> out [rows_pad, 2048], weights resident in registers, rows
// streamed; bit-identical to launch_conv on the same plan.  p: c->xproj[l] (reads the packed image and bias as they are).  rows_pad: a
// multiple of 256.  hipErrorNotSupported for any other plan or shape: the caller runs the conv route.
struct SeqProjPlan { int grid, chunks, ring; long long nslots, chunk_slots; };   // workgroups, row chunks (grid / 4), slots of the LDS ring, 64-row slots in all / per chunk
SeqProjPlan seq_proj_plan(size_t rows_pad, int ncu);                        // chunk i covers slots [i * chunk_slots, min(nslots, (i + 1) * chunk_slots))
hipError_t launch_seq_proj(const ConvPlan& p, const uint16_t* x, size_t rows_pad, uint16_t* out, hipStream_t s);
// ---- rec_quant (quant.hip): the sequence half in torch's dynamic int8 arithmetic, per crop.  seqs_dev: int2 {first row, T} per crop (the CTC
// stage's table).  launch_q8_quantize: parameter + coding pass over x (src_pair 0: fp32 [rows, K]; 1: the exact mode's fp16 pair [rows, K | K]) ->
// rowp float4 [rows_pad] {scale, 1 / scale, zero point, 0}, a8 int8 [rows_pad, K] = code - zero point (rows past `rows` cleared), optionally the
// codes uint8 [rows, K] and segp float2 [nseq] {scale, zero point}.  launch_q8_gemm: out fp32 [rows_pad, ldo] = fmaf(acc, rowp.scale *
// wscale[col / 16], bias[col]) over N columns (N % 64 == 0, or 112 with K = 256) of weights packed by pack_q8_weights.
size_t q8_packed_bytes(int N, int K);
void pack_q8_weights(const int8_t* q /*[N][K]*/, int N, int K, int8_t* out);
void pack_q8_whh(const int8_t* q_fwd, const int8_t* q_bwd /*[1024][256]*/, int8_t* out /*2 x 256 KB*/);
hipError_t launch_q8_quantize(const void* x, int src_pair, int K, size_t rows, size_t rows_pad, const int* seqs_dev, int nseq, float* rowp, int8_t* a8,
                              uint8_t* codes, float* segp, hipStream_t s);
hipError_t launch_q8_gemm(const int8_t* a8, size_t rows_pad, int K, const int8_t* wpk, int N, const float* rowp, const float* wscale, const float* bias,
                          float* out, int ldo, hipStream_t s);
// G fp32 [rows, 2048] (column dir * 1024 + gate * 256 + unit) -> out fp32 [rows, 512] (fwd | bwd).  tiles_dev: int4 {first sequence, sequences
// (1..16), longest T, 0} per workgroup, indexing seqs_dev.  whh_scale [2], bhh [2][1024].  Optional, row-indexed like out: c_out (the cell state),
// hcodes uint8 [rows, 512] and hparams float2 [rows][2] = codes and {scale, zero point} of the h that ENTERED that step.
constexpr int LSTM_Q8_SEQS = 16;
hipError_t launch_lstm_q8(const float* G, const int8_t* whh_pk, const float* whh_scale, const float* bhh, float* out, const int* seqs_dev,
                          const int* tiles_dev, int ntiles, float* c_out, uint8_t* hcodes, float* hparams, hipStream_t s);
struct CtcOut { int len; int cnt; float prod; int pad; };
// seqs_dev: int2 per sequence {first row, T}; logits fp32 [rows, cs]; out_idx is row-indexed like the pool
hipError_t launch_ctc(const float* logits, size_t rows, int C, int cs, const int* seqs_dev, int nseq, int* idx_tmp, float* pmax_tmp,
                      int* out_idx, CtcOut* out, hipStream_t s, const unsigned int* ignore = nullptr, float* probs_out = nullptr);   // ignore: 4 x 32-bit class mask or null
// the same stage over MORE than 128 classes (ctc_rows_wide_kernel: one wavefront per row, classes strided over the lanes 64 at a time, so every
// load is 256 contiguous bytes), then ctc_collapse_kernel as above.  mask_dev: ceil(C / 32) words on the device (bit c of word c >> 5 removes
// class c) or null.  Columns >= C of a row are neither read nor written.
hipError_t launch_ctc_wide(const float* logits, size_t rows, int C, int cs, const int* seqs_dev, int nseq, int* idx_tmp, float* pmax_tmp,
                           int* out_idx, CtcOut* out, hipStream_t s, const unsigned int* mask_dev = nullptr, float* probs_out = nullptr);
// ctc_collapse_kernel alone, over idx / pmax that another kernel wrote (pred_ctc.hip)
hipError_t launch_ctc_collapse(const int* idx, const float* pmax, const int* seqs_dev, int nseq, int* out_idx, CtcOut* out, hipStream_t s);
// Prediction + softmax + mask + arg-max as one kernel that stores no logits (pred_ctc.hip): x [rows, 256] 16-bit elements of type el, wpk / bias
// from pack_pred_ctc_weights -> idx [rows], pmax [rows].  C > 128 is what it is built for; any C >= 2 is computed.
constexpr int kPredCtcRows = 64;                       // rows of x a workgroup keeps in registers
size_t pred_ctc_packed_elems(int C);                   // 16-bit elements of the packed weights: ceil(C / 16) fragments x 8 k-steps x 64 lanes x 8
size_t pred_ctc_bias_elems(int C);
void pack_pred_ctc_weights(int el, const float* w /* [C][256] */, const float* b /* [C] */, int C, uint16_t* wpk, float* bias);
hipError_t launch_pred_ctc(int el, const uint16_t* x, size_t rows, const uint16_t* wpk, const float* bias, int C, const unsigned int* mask_dev,
                           int* idx, float* pmax, hipStream_t s);
// decoder='beamsearch' (easyocr/utils.py::ctcBeamSearch, host: the definition, and the path of beams wider than BBOCR_BEAM_DEVICE_MAX): probs fp32 [rows, cs] as ctc_rows_kernel writes them; seqs = {first row, T}
void ctc_beam_search_host(const float* mat, int T, int C, int cs, int beam_width, std::vector<int>& text);
class HostPool;
void ctc_beam_search_batch(const float* probs, const int* seqs, int nseq, int C, int cs, int beam_width, std::vector<std::vector<int>>& texts,
                           HostPool* pool = nullptr);     // pool: the calling slot's workers (null: the calling thread alone)
// the same search on the device (ctc_beam.hip), one wave per sequence: text of sequence i into out_text[first row of i ...] (row-indexed like
// launch_ctc's out_idx), its length into out_len[i].  max_T: the longest T of the table (sizes the labellings' LDS block).  Widths above
// BBOCR_BEAM_DEVICE_MAX or tables whose LDS block would pass kCtcBeamLdsLimit are hipErrorInvalidValue: ask ctc_beam_on_device first.
constexpr size_t kCtcBeamLdsLimit = 65536;
size_t ctc_beam_lds_bytes(int beam_width, int C, int max_T);
bool ctc_beam_on_device(int beam_width, int C, int max_T);
hipError_t launch_ctc_beam(const float* probs, size_t rows, int C, int cs, const int* seqs_dev, int nseq, int max_T, int beam_width, int* out_text,
                           int* out_len, hipStream_t s);
// decoder='wordbeamsearch' (ctc_wordbeam.cpp states it; word_dict.h: the dictionary).  Host: one sequence / a {first row, T} table; dict null
// or empty: every word group decodes as ctc_beam_search_host decodes its rows
struct WdTable;
void ctc_wordbeam_search_batch(const float* probs, const int* seqs, int nseq, int C, int cs, int beam_width, int space, const WdTable* dict,
                               std::vector<std::vector<int>>& texts, HostPool* pool = nullptr);
// ... and on the device (ctc_wordbeam.hip), C <= 128: the table as uploaded (WdSlot slots, byte symbols), word groups from the rows' arg-max
// (segs {first row, T} x seg_cap, seq_seg {first segment, count} per sequence, *counter their total), one wave per group, then the join into
// out_text (row-indexed) / out_len.  seg_text (row-indexed like out_text) and seg_len (seg_cap) are the stage in between.  seg_cap: at least
// the sum of (T + 1) / 2 over the sequences.  Ask ctc_wordbeam_on_device first (width, classes, LDS block of the longest SEQUENCE).
struct WordDictDev { const void* slots = nullptr; const unsigned char* pool = nullptr; unsigned int nslots = 0, pool_n = 0; int probe = 0; };
size_t ctc_wordbeam_lds_bytes(int beam_width, int C, int max_T);
bool ctc_wordbeam_on_device(int beam_width, int C, int max_T);
hipError_t launch_row_argmax(const float* probs, size_t rows, int C, int cs, int* idx, hipStream_t s);
hipError_t launch_word_segments(const int* idx, size_t rows, const int* seqs_dev, int nseq, int space, int* segs, int seg_cap, int* seq_seg, int* counter,
                                hipStream_t s);
hipError_t launch_ctc_wordbeam(const float* probs, size_t rows, int C, int cs, const int* seqs_dev, int nseq, int max_T, int beam_width, int space,
                               const WordDictDev& d, const int* segs, int seg_cap, const int* seq_seg, const int* counter, int* seg_len, int* seg_text,
                               int* out_text, int* out_len, hipStream_t s);
hipError_t launch_dict_lookup(const WordDictDev& d, const unsigned char* qsym, const int* qoff, int nq, int qtotal, int* found, hipStream_t s);
// the device search for 128 < C <= BBOCR_REC_CLASSES_MAX (ctc_beam_wide.hip; bbocr_config_v2::beam_wide): ctc_beam_cand_kernel lists every row's
// candidates (cand_n int32 [rows]: the count; cand [rows][kBeamWideCand] {class, p bits}: the first kBeamWideCand of them, ascending), then
// ctc_beam_wide_kernel searches one sequence per wave from that list and the two values it gathers from the full row.  Outputs as
// launch_ctc_beam's, except that a sequence with a row of more than kBeamWideCand candidates gets out_len = -1 and no text: the caller
// searches it on the host.  Ask ctc_beam_wide_on_device first (width, class range, LDS block of the longest sequence).
constexpr int kBeamWideCand = 128;
size_t ctc_beam_wide_lds_bytes(int beam_width, int max_T);
bool ctc_beam_wide_on_device(int beam_width, int C, int max_T);
hipError_t launch_ctc_beam_wide(const float* probs, size_t rows, int C, int cs, const int* seqs_dev, int nseq, int max_T, int beam_width, int* cand_n,
                                int* cand, int* out_text, int* out_len, hipStream_t s);

// ------------------------------------------------------------------ OCR pre-processing chain (preproc.hip), SURVEY 8 row f2
// Which kernel a launcher of the chain takes (include/bbocr.h BBOCR_PP_*, same order): decided by the pp_*_route functions below from the
// plane's size and the low two bits of the pointers alone; the launchers switch on the same functions.
enum PpRoute : int {
    PP_GAUSS_X4 = 0, PP_GAUSS_BYTE,
    PP_HIST_X4, PP_HIST_BYTE,
    PP_APPLY_CELL_2, PP_APPLY_CELL_8, PP_APPLY_CELL_32, PP_APPLY_VEC, PP_APPLY_BYTE,
    PP_BOX0_X4, PP_BOX_BYTE,
    PP_UNSHARP_FUSED, PP_UNSHARP_PASSES_VEC, PP_UNSHARP_PASSES_BYTE,
    PP_RESIZE_TILED32, PP_RESIZE_TILED16, PP_RESIZE_PIXEL,
    PP_ROUTE_COUNT
};
int pp_resize_tile_rows(int H, int W, int dh, int dw);
PpRoute pp_resize_route(int H, int W, int dh, int dw);
bool pp_resize_dword_rows(int dw, unsigned dst_bits);
PpRoute pp_gauss_route(int H, int W, unsigned src_bits, unsigned dst_bits);
PpRoute pp_clahe_hist_route(int H, int W, unsigned src_bits);
PpRoute pp_clahe_apply_route(int H, int W, int th, unsigned src_bits, unsigned dst_bits);
PpRoute pp_box_route(int H, int W, int r, unsigned src_bits, unsigned dst_bits);
PpRoute pp_unsharp_route(int H, int W, int r, unsigned src_bits, unsigned tmp_bits, unsigned dst_bits);
hipError_t launch_pp_resize_cubic(const uint8_t* src, int H, int W, uint8_t* dst, int dh, int dw, const int* x0, const double* wx, const long long* nx,
                                  const int* y0, const double* wy, const long long* ny, unsigned long long KX, unsigned long long KY, hipStream_t s, int src_bgr = 0);
hipError_t launch_pp_gauss3(const uint8_t* src, int H, int W, uint8_t* dst, int k0, int k1, int k2, unsigned long long* sum, hipStream_t s);
hipError_t launch_pp_clahe_hist(const uint8_t* src, int H, int W, const uint8_t* lut, int tw, int th, int tx, int ty, unsigned int* hist,
                                hipStream_t s);
hipError_t launch_pp_clahe_apply(const uint8_t* src, int H, int W, const uint8_t* lut, const uint8_t* tile_luts, int tw, int th, int tx, int ty,
                                 uint8_t* dst, hipStream_t s);
hipError_t launch_pp_box_pass(const uint8_t* src, uint8_t* dst, int H, int W, int vertical, int r, unsigned int ww, unsigned int fw, hipStream_t s);
hipError_t launch_pp_fold_lut(const unsigned long long* sum, unsigned long long n, float contrast, float brightness, uint8_t* lut, hipStream_t s);
hipError_t launch_pp_clahe_luts(const unsigned int* hist, int tiles, int clip, float lut_scale, uint8_t* tile_luts, hipStream_t s);
hipError_t launch_pp_lut(const uint8_t* src, uint8_t* dst, const uint8_t* lut, size_t total, hipStream_t s);
hipError_t launch_pp_unsharp_fused(const uint8_t* in, uint8_t* tmp, uint8_t* dst, int H, int W, unsigned int ww, unsigned int fw, int percent,
                                   int threshold, hipStream_t s);
hipError_t launch_pp_unsharp(const uint8_t* in, const uint8_t* blur, uint8_t* dst, size_t total, int percent, int threshold, PpRoute route,
                             hipStream_t s);

// ------------------------------------------------------------------ text-region auto-crop (autocrop.hip), enhanced_extractor.py::_auto_crop_text_region
constexpr int AC_BOX = 35, AC_BOX_R = 17, AC_MEAN_C = 10;     // adaptiveThreshold MEAN: block 35, C 10
constexpr int AC_GAU = 31, AC_GAU_R = 15, AC_GAU_C = 5;       // adaptiveThreshold GAUSSIAN: block 31, C 5
struct AcTaps { int k[AC_GAU]; };                             // 8.8 fixed-point Gaussian taps (sum 256)
hipError_t launch_ac_gray_blur(const uint8_t* src, int H, int W, size_t pitch, int channels, uint8_t* dst, hipStream_t s);
hipError_t launch_ac_cues(const uint8_t* e, int H, int W, const AcTaps& taps, uint16_t* rbox, uint16_t* rgau, uint8_t* part, uint8_t* grad,
                          unsigned int* hist, int* thr, hipStream_t s);
hipError_t launch_ac_pack(const uint8_t* e, const uint8_t* part, const uint8_t* grad, const int* thr, int H, int W, int WW, uint32_t* bits, hipStream_t s);
hipError_t launch_ac_pack_mask(const uint8_t* src, size_t pitch, int H, int W, int WW, uint32_t* bits, hipStream_t s);
hipError_t launch_ac_rect(const uint32_t* src, uint32_t* tmp, uint32_t* dst, int H, int W, int WW, int rx, int ry, int erode, const uint32_t* or_with,
                          hipStream_t s);
hipError_t launch_ac_components(const uint32_t* bits, int H, int W, int WW, int* label, uint8_t* flag, int* count, int cap, int* boxes, hipStream_t s);
hipError_t launch_ac_unpack(const uint32_t* bits, const int* label, int H, int W, int WW, uint8_t* dst, hipStream_t s);

// ------------------------------------------------------------------ device pages: rows of packed pixels, the layouts of bbocr.h BBOCR_PAGE_*
enum : int { PAGE_GRAY = 0, PAGE_BGR = 1, PAGE_RGB = 2, PAGE_YCC4 = 3, PAGE_YCC3 = 4 };
__host__ __device__ constexpr int page_px_bytes(int layout) { return layout == PAGE_GRAY ? 1 : (layout == PAGE_YCC4 ? 4 : 3); }

// ------------------------------------------------------------------ pages of mixed shapes -> the detector's and the recogniser's inputs (pages.hip)
constexpr int PK_TILE_PX = 4096;                               // pixels per workgroup of the pack kernel: 16 per lane
constexpr int PK_MAX_TILES = (1 << 24) - 1;                    // HIP launches fewer than 2^32 threads per grid dimension: 256 * tiles < 2^32
struct PackPage {                                              // one page of a bbocr_readtext_pages call, as the pack kernel reads it
    const uint8_t* rgb;                                        // [H][W][3], rows rgb_pitch bytes apart
    const uint8_t* gray;                                       // [H][W], rows gray_pitch apart, or null: derived from rgb (bgr2gray_px)
    long long rgb_pitch, gray_pitch;
    long long rgb_off, gray_off;                               // byte offsets of the page's tight copies in the two staging buffers
    int H, W;
    int tile0;                                                 // first tile of this page in the flat tile list (ceil(H * W / PK_TILE_PX) tiles each)
    int vec;                                                   // bit 0: RGB copy, bit 1: gray plane -- 16-byte accesses (pointers, pitches and offsets allow them)
};
int pack_page_vec(const PackPage& g, const uint8_t* rgb_staging, const uint8_t* gray_staging);   // the `vec` bits of a page whose other fields are set, for these staging buffers
// every page's RGB tight into rgb_staging + rgb_off and its gray plane (given or derived) tight into gray_staging + gray_off: ONE launch over
// the flat tile list of all n pages (ntiles = tile0 + tiles of the last page); pages_dev: the table on the device
hipError_t launch_pack_pages(const PackPage* pages_dev, int n, int ntiles, uint8_t* rgb_staging, uint8_t* gray_staging, hipStream_t s);

// ------------------------------------------------------------------ OCR-input thumbnail + JPEG round trip (thumb.hip), enhanced_extractor.py:486-512
constexpr int TH_PRECISION_BITS = 22;                                             // Pillow Resample.c, 8 bpc
struct ThQuant { unsigned short q[2][64]; };                                       // luminance, chrominance (natural order)
hipError_t launch_th_reduce(const uint8_t* src, size_t pitch, int layout, int H, int W, int fx, int fy, uint8_t* dst, int rh, int rw, int C,
                            hipStream_t s);
hipError_t launch_th_resample_h(const uint8_t* src, size_t pitch, int layout, int y0, int rows, int ow, int C, const int* bounds, const int* kk,
                                int ksize, uint8_t* dst, hipStream_t s);
hipError_t launch_th_resample_v(const uint8_t* src, size_t spitch, int y0, int width, int oh, const int* bounds, const int* kk, int ksize,
                                uint8_t* dst, size_t dpitch, hipStream_t s);
hipError_t launch_th_jpeg(const uint8_t* src, size_t pitch, int C, int H, int W, const ThQuant& q, uint8_t* yp, int wp, uint8_t* cbp, uint8_t* crp,
                          hipStream_t s);
hipError_t launch_th_upsample(const uint8_t* yp, int wp, const uint8_t* cbp, const uint8_t* crp, int H, int W, int gray_only, uint8_t* rgb,
                              uint8_t* gray, uint8_t* ycc, hipStream_t s);
hipError_t launch_th_direct(const uint8_t* src, size_t pitch, int layout, int H, int W, uint8_t* rgb, uint8_t* gray, hipStream_t s);

// ------------------------------------------------------------------ baseline JPEG encoder (jpegenc.hip): the file Pillow saves, from a device page
// Passes: coefficients (one MCU per wavefront) -> bit length per block + scan inside tiles of JE_TILE blocks -> scan of the tile sums
// -> packing -> 0xFF count per tile of JE_STUFF_TILE bytes -> scan of those -> scatter with the stuffed zero bytes.
constexpr int JE_TILE = 256;                                   // blocks per workgroup of the size and packing passes
constexpr int JE_STUFF_TILE = 2048;                            // scan bytes per workgroup of the stuffing passes
constexpr int JE_BLOCK_MAX_BITS = 22 + 63 * 26;                // DC: 11-bit code + 11 bits; 63 x (16-bit code + 10 bits)
struct JeHuff { uint32_t dc[2][16], ac[2][256]; };             // luminance, chrominance: (code << 5) | length per symbol, 0 = no code
struct JeStdTable { unsigned char bits[16], vals[162]; int n; };
// ITU T.81 Annex K.3, in the order libjpeg writes them: DC luminance, AC luminance, DC chrominance, AC chrominance
constexpr JeStdTable JE_STD[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
      0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
      0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
      0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
      0xFA}, 162},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
      0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
      0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
      0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
      0xFA}, 162},
};
constexpr JeHuff je_std_huff() {                               // Annex C: codes of increasing length, counted up within a length
    JeHuff h{};
    for (int t = 0; t < 4; ++t) {
        uint32_t* out = (t & 1) ? h.ac[t >> 1] : h.dc[t >> 1];
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < JE_STD[t].bits[len - 1]; ++i) out[JE_STD[t].vals[k++]] = (code++ << 5) | (uint32_t)len;
            code <<= 1;
        }
    }
    return h;
}
inline int je_blocks(int H, int W, int components) {            // blocks in the scan
    return components == 1 ? ((H + 7) / 8) * ((W + 7) / 8) : 6 * ((H + 15) / 16) * ((W + 15) / 16);
}
// coef [blocks][64] int16 zig-zag, blocks in MCU order; `components` 1 (a gray page) or 3 (any layout; a gray page: zero chroma blocks)
hipError_t launch_je_coef(const uint8_t* src, size_t pitch, int layout, int components, int H, int W, const ThQuant& q, short* coef, hipStream_t s);
// local [n]: bit offset of block b inside its tile of JE_TILE blocks; tile_bits [tiles + 1]: the tiles' bit counts (the scan below turns
// them into offsets)
hipError_t launch_je_sizes(const short* coef, int n, int components, unsigned int* local, unsigned long long* tile_bits, hipStream_t s);
// v [n + 1]: exclusive prefix sum in place, the total in v[n]; one workgroup
hipError_t launch_je_scan(unsigned long long* v, int n, hipStream_t s);
hipError_t launch_je_offsets(const unsigned int* local, const unsigned long long* tile_off, int n, long long* out, hipStream_t s);   // [n + 1]
// words: zeroed, ceil(total bits / 32) words; the last byte of the scan is filled with 1-bits
hipError_t launch_je_pack(const short* coef, int n, int components, const unsigned int* local, const unsigned long long* tile_off, uint32_t* words,
                          hipStream_t s);
hipError_t launch_je_ff_count(const uint8_t* scan, long long bytes, unsigned long long* tile_ff, hipStream_t s);       // [tiles + 1]
hipError_t launch_je_stuff(const uint8_t* scan, long long bytes, const unsigned long long* tile_off, uint8_t* out, hipStream_t s);

// ------------------------------------------------------------------ lossless PNG writer (pngenc.hip): filters, run matches, dynamic Huffman per chunk
// Passes: adaptive filter per row -> per chunk of PNG_CHUNK stream bytes: tokens, histogram, code lengths, block size, Adler-32 sums
// -> scan of the chunk sizes (launch_je_scan) -> per chunk: bit packing in LDS, written at the chunk's place in the compacted buffer.
// tests/png_ref.py states every rule; the device is held to it byte for byte.
constexpr int PNG_CHUNK = 16384;                               // BBOCR_PNG_CHUNK: stream bytes per deflate block; no match leaves its chunk
constexpr int PNG_LITLEN = 286, PNG_CL = 19;                   // literal/length symbols, code-length symbols (RFC 1951)
constexpr int PNG_HIST_ROW = 288;                              // uint32 per chunk: 286 symbol counts, the match count, the token count
constexpr int PNG_REC = 320;                                   // bytes per chunk record, see PngRec
constexpr int PNG_STORED = 0, PNG_DYNAMIC = 1;
constexpr int PNG_LIMIT15 = 1, PNG_LIMIT7 = 2;                 // PngRec::flags: a code was deeper than its limit before the limiter ran
struct PngRec {                                                // what the packing pass reads of a chunk (bbocr_op_png_stage stage 2)
    uint8_t kind, flags;
    uint8_t litlen[PNG_LITLEN];                                // code lengths, 0 = unused
    uint8_t dist;                                              // length of distance symbol 0: 1 when the chunk has matches, else 0
    uint8_t cl[PNG_CL];                                        // lengths of the code-length code, in symbol order
    uint8_t pad[PNG_REC - 2 - PNG_LITLEN - 1 - PNG_CL];
};
static_assert(sizeof(PngRec) == PNG_REC, "PngRec layout");
// the filtered stream of a page: per row [filter byte][W * c bytes], c = 1 (gray) or 3 (RGB order; a BGR page is swapped on read)
hipError_t launch_png_filter(const uint8_t* src, size_t pitch, int layout, int H, int W, uint8_t* stream, hipStream_t s);
// hist [chunks][PNG_HIST_ROW], rec [chunks], size [chunks + 1] (bytes of each chunk's block; the scan turns them into offsets), adler [chunks][2]
hipError_t launch_png_codes(const uint8_t* stream, size_t n, int chunks, uint32_t* hist, PngRec* rec, unsigned long long* size, uint32_t* adler,
                            hipStream_t s);
hipError_t launch_png_pack(const uint8_t* stream, size_t n, int chunks, const PngRec* rec, const unsigned long long* off, uint8_t* out, hipStream_t s);

// ------------------------------------------------------------------ EXIF orientation + colour order of a page (orient.hip): cv2.imread's last step
constexpr int ORIENT_TILE = 64;                                // pixels per tile edge (bb_ocr_amd.preprocess.ORIENT_TILE: the tests' shapes)
bool page_orient_pair_ok(int layout, int dst_layout);          // BGR / RGB from every PAGE_* layout, GRAY from GRAY
// src [H,W] pixels of `layout`, rows `pitch` apart -> dst in `dst_layout`, [H,W] (orientation 1-4) or [W,H] (5-8), rows `dst_pitch` apart
hipError_t launch_page_orient(const uint8_t* src, int H, int W, size_t pitch, int layout, int orientation, int dst_layout, uint8_t* dst,
                              size_t dst_pitch, hipStream_t s);

// ------------------------------------------------------------------ baseline JPEG decoder (jpegdec.hip): speculative Huffman decoding with self-synchronisation
constexpr int JD_LANES = 64;                                   // subsequences per workgroup of the synchronisation and write passes
constexpr int JD_SUBSEQ_BITS = 1024;                           // default subsequence length
struct JpegHuff {                                              // one Huffman table as the lanes read it from LDS (jdhuff.c's derived table)
    unsigned short look[512];                                  // 9-bit look-ahead: (length << 8) | symbol, 0 = the code is longer (or none)
    int maxcode[18];                                           // largest code of length l, -1 = none
    int valoff[18];                                            // index of the first symbol of length l minus its code
    unsigned char val[256];
};
// How the output stage brings a component's plane to the output's size.  The first five are include/bbocr.h's BBOCR_JPEG_UP_* (pinned in
// jpegdec.cpp); a decode at scale 1 of a 4:2:0 file adds the sixth.
enum : int { JD_UP_NONE = 0, JD_UP_H2V1_FANCY = 1, JD_UP_H1V2_FANCY = 2, JD_UP_H2V2_NOT_NEEDED = 3, JD_UP_REPLICATE = 4, JD_UP_H2V2_FANCY = 5 };
struct JpegComp {                                              // one component's plane in one IDCT + output pass (jpegdec.cpp's jpeg_geometry)
    int n;                                                     // edge of one block's samples: 8, 4, 2 or 1
    int bw, bh;                                                // the component's blocks of an MCU across / down
    int plane_rows, pitch;                                     // the plane in whole MCUs: mcuy * bh * n rows of pitch = mcux * bw * n samples
    int valid_rows, valid_cols;                                // the extent the output stage reads
    int up;                                                    // JD_UP_*
};
struct JpegSubs {                                              // a scan cut into subsequences of S bits for the speculative passes (jpeg_spec.h)
    const uint8_t* data;                                       // entropy-coded bytes without stuffing and restart markers, segment after segment
    const int* seg_byte;                                       // [nseg + 1] first byte of each segment in `data`
    const int* seg_sub;                                        // [nseg + 1] first subsequence of each segment
    const int* sub_seg;                                        // [nsub] segment of each subsequence
    unsigned long long* entry;                                 // [nsub] packed state (jpeg_pack) a lane starts from / ends in
    unsigned long long* exits;
    int* count;                                                // [nsub] blocks completed by the subsequence
    int* scan;                                                 // [nsub] exclusive scan of count over the scan
    int* flags;                                                // [passes] flags[k] != 0: synchronisation pass k changed a state
    int nseg, nsub, S, passes;
};
struct JpegDesc : JpegSubs {                                   // one file of a batch and its one scan; every pointer is device memory
    int* first;                                                // [nsub] first output block (written by the write pass)
    int* status;                                               // JD_ERR_* bits
    short* coef;                                               // [nblocks][64] natural order, MCU block order
    uint8_t* plane[3];                                         // Y, Cb, Cr of this pass: comp[c].plane_rows rows of comp[c].pitch samples
    uint8_t* out;                                              // this pass's pixels: OH rows of OW, rows `pitch` bytes apart
    long long pitch;
    JpegComp comp[3];                                          // this pass's geometry: all the IDCT and the output stage know of sampling and scale
    int OW, OH;
    const JpegHuff* huff;                                      // [4]: DC 0, DC 1, AC 0, AC 1
    const unsigned short* quant;                               // [ncomp][64] natural order
    int W, H, ncomp, bpm, mcux, mcuy, nmcu, ri, nblocks, px;
    int hs, vs;                                                // luma blocks of an MCU across / down: bpm = hs * vs + 2 (1 component: 1, 1, bpm 1)
    int tab_dc[3], tab_ac[3];                                  // per component: index into huff
};
enum : int { JD_ERR_SYNC = 1, JD_ERR_CODE = 2, JD_ERR_COUNT = 4 };
hipError_t launch_jd_sync(const JpegDesc* descs, int n, int max_groups, int pass, hipStream_t s);
hipError_t launch_jd_scan(const JpegDesc* descs, int n, hipStream_t s);
hipError_t launch_jd_write(const JpegDesc* descs, int n, int max_groups, hipStream_t s);
hipError_t launch_jd_dc(const JpegDesc* descs, int n, int max_seg, hipStream_t s);
// One IDCT + output pass over descs[0 .. n) (one descriptor per file and pass): every block through the transform of its component's edge
// into the component's plane, then the planes -> OW x OH pixels at `out`.  max_blocks, max_h, max_w: the largest nblocks, OH, OW of the pass.
hipError_t launch_jd_idct(const JpegDesc* descs, int n, int max_blocks, hipStream_t s);
hipError_t launch_jd_output(const JpegDesc* descs, int n, int max_h, int max_w, hipStream_t s);
