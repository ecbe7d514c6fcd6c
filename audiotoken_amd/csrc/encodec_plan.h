// Acoustic tokenizer: what a call does, decided before anything is launched. The workspace plans of encode / decode and of their streams, the stream-state
// layouts, the options, and the kernel ROUTE of a call as a pure function of (options, plan). Host code only: no HIP call, no device pointer.
#pragma once
#include <cstddef>
#include <cstdlib>

namespace at {

constexpr int kRatiosEnc[4] = {2, 4, 5, 8};
constexpr int kRatiosDec[4] = {8, 5, 4, 2};
constexpr int kH = 512;
constexpr int kDim = 128;
constexpr int kCodes = 1024;
constexpr int kPipeMaxClips = 80;   // lstm_pipe.hip: 5 groups of 16 clips x 48 workgroups on 256 CUs (the launcher checks the device)
constexpr int kSubBatchDefault = 256;  // clips per pass through the 24 kHz..75 Hz conv stack (bounds the workspace)
inline int sub_batch() {
    static const int v = [] {
        const char* e = std::getenv("AUDIOTOKEN_SUBBATCH");
        const int n = e ? std::atoi(e) : 0;
        return n > 0 ? n : kSubBatchDefault;
    }();
    return v;
}

// The boolean options of a handle (at_encodec_set_option / at_encodec_get_option, by these names).
struct Options {
    bool fused_stage0 = true;       // conv0 + resblock + strided conv in one kernel (seanet_stage0.hip)
    bool fused_res64 = true;        // 64-channel residual block in one kernel (seanet_res64.hip)
    bool fused_res128 = true;       // 128-channel residual block in one kernel (seanet_res128.hip)
    bool fused_down64 = true;       // stage-1 strided conv with register-stationary weights (seanet_down64.hip)
    bool fused_stage1 = true;       // 64-channel block + stage-1 strided conv in one role-split kernel (seanet_res64down.hip; fp16 scheme, needs res64_x3 / down64_x3 / res_f16x2)
    bool down64_x3 = true;          // ... on the bf16 matrix cores with 3-way split operands (seanet_down64x3.hip); follows bf16x3
    bool down128_x3 = true;         // stage-2 strided conv as a windowed split-bf16 GEMM fed by seanet_res128x3's split epilogue; follows bf16x3
    bool rvq_x3 = true;             // RVQ search with the dot products on the bf16 matrix cores (rvq_encode_x3.hip); follows bf16x3
    bool fin_f16x2 = true;          // final conv as a windowed GEMM on two fp16 pieces
    bool up_f16x2 = true;           // decoder transposed convs as two-tap windowed GEMMs on two fp16 pieces
    bool res128_rs = true;          // 128-channel block (fp16 scheme): the role-split kernel (seanet_res128rs.hip) instead of seanet_res128x3.hip; same bits
    bool rvq_f16x2 = true;          // RVQ search on two fp16 pieces of the codebooks
    bool lstm_x3 = true;            // persistent LSTM with the recurrent product on the bf16 matrix cores (lstm_seq_x3.hip); follows bf16x3
    bool res256_x3 = true;          // 256-channel block as two split-bf16 GEMMs chained between the stage-2 and stage-3 strided convs; follows bf16x3
    bool down256_x3 = true;         // stage-3 strided conv as a windowed split-bf16 GEMM behind a split pass; follows bf16x3
    bool stage0_x3 = true;          // fused stage 0 on the bf16 matrix cores (seanet_stage0x3.hip); follows bf16x3
    bool res64_x3 = true;           // 64-channel residual block on the bf16 matrix cores (seanet_res64x3.hip); follows bf16x3
    bool res128_x3 = true;          // 128-channel residual block on the bf16 matrix cores (seanet_res128x3.hip); follows bf16x3
    bool fused_dectail = true;      // decoder: last transposed conv + block + final conv in one kernel (seanet_dectail.hip)
    bool tail_f16x2 = true;         // ... with its contractions on the two-piece fp16 scheme (seanet_dectail_x2.hip)
    bool dec_chain = true;          // decoder stage 0 (256 channels): the block as two split GEMMs whose output is the next transposed conv's operand (seanet_dec256.hip)
    bool chain_f16x2 = true;        // the stage 2-3 GEMM chain on two fp16 pieces (else three bf16 pieces)
    bool res_f16x2 = true;          // fused residual blocks on the fp16 scheme
    bool lstm_f16x2 = true;         // LSTM recurrence on the fp16 scheme
    bool lstm_pipe = true;          // batches of <= 80 clips: both LSTM layers in one pipelined launch (lstm_pipe.hip), same arithmetic
    bool ih_f16x2 = true;           // LSTM input projections on the fp16 scheme (three MFMA products instead of six)
    bool dec_skip_twin = false;     // one-shot decode and a stream's first push store through the skip / stride tail variants with skip = 0 and a dense stride (the A/B twin of the tests)
    bool persistent_lstm = false;   // whole-sequence persistent LSTM (needs one resident workgroup per CU for 256 CUs)
};

inline int out_len(int L, int stride) { return (L + stride - 1) / stride; }

struct EncPlan {
    int L[5];        // lengths: L[0] = N, L[s+1] = ceil(L[s]/ratio)
    int G;           // sub-batch
    size_t off_x[4], off_h[4], off_r[4];  // per-stage sub-batch buffers (floats)
    size_t off_x4, off_xg, off_xg2, off_h0, off_h1, off_c, off_y, off_emb, off_sync, off_xs;
    int Mpf = 0, Lpf = 0;   // final conv as a windowed GEMM: padded output rows / operand rows per clip
    int Mp3, Lp3; size_t off_s3;   // stage-3 strided conv the same way, its input split by a separate pass or by the block's tail GEMM
    int Mpc, Lpc; size_t off_ac3, off_at3;   // 256-channel block as two split-bf16 GEMMs: pieces of ELU(x) (2 front rows) and of [h | x]
    int Mp2, Lp2;    // stage-2 strided conv as a windowed split-bf16 GEMM: padded output rows, rows per phase plane of its input pieces
    size_t total_floats;
};

inline EncPlan make_plan(int B, int N, int sub) {
    EncPlan p;
    p.L[0] = N;
    for (int s = 0; s < 4; ++s) p.L[s + 1] = out_len(p.L[s], kRatiosEnc[s]);
    p.G = B < sub ? B : sub;
    size_t cur = 0;
    auto take = [&](size_t n) { size_t o = cur; cur += (n + 63) / 64 * 64; return o; };
    for (int s = 0; s < 4; ++s) {
        const size_t C = 32u << s;
        p.off_x[s] = take((size_t)p.G * p.L[s] * C);
        p.off_h[s] = take((size_t)p.G * p.L[s] * (C / 2));
        size_t rn = (size_t)p.G * p.L[s] * C;
        if (s == 2) {   // r[2] doubles as the K-blocked phase-major bf16 pieces of ELU(block output) (3 pieces x 2 B = 1.5 floats per element)
            p.Mp2 = (p.L[3] + 255) / 256 * 256;
            const int reach = p.Mp2 + (10 - 1) / 5, have = (p.L[2] + 5 + 4) / 5;
            p.Lp2 = ((have > reach ? have : reach) + 63) / 64 * 64;
            const size_t pn = (size_t)p.G * 5 * p.Lp2 * C * 3 / 2 + 64;
            rn = pn > rn ? pn : rn;
        }
        p.off_r[s] = take(rn);
    }
    {
        p.Mp3 = (p.L[4] + 255) / 256 * 256;
        const int reach = p.Mp3 + (16 - 1) / 8, have = (p.L[3] + 8 + 7) / 8;
        p.Lp3 = ((have > reach ? have : reach) + 63) / 64 * 64;
        p.off_s3 = take((size_t)p.G * 8 * p.Lp3 * 256 * 3 / 2 + 64);
        p.Mpc = (p.L[3] + 255) / 256 * 256;
        p.Lpc = (p.Mpc + 2 + 63) / 64 * 64;
        p.off_ac3 = take((size_t)p.G * p.Lpc * 256 * 3 / 2 + 64);
        p.off_at3 = take((size_t)p.G * p.Mpc * 384 * 3 / 2 + 64);
    }
    const size_t T = p.L[4];
    p.off_x4 = take((size_t)B * T * kH);
    p.off_xg = take((size_t)B * T * 4 * kH);
    p.off_xg2 = take(B <= kPipeMaxClips ? (size_t)B * T * 4 * kH : 0);   // layer-2 input gates of the pipelined LSTM launch (small batches)
    p.off_h0 = take((size_t)B * T * kH);
    p.off_h1 = take((size_t)B * T * kH);
    p.off_c = take((size_t)B * kH);
    p.off_y = take((size_t)B * T * kH);
    p.off_emb = take((size_t)B * T * kDim);
    p.off_sync = take(1024);
    // split copy of an LSTM layer's input (three bf16 pieces at most); the same region then holds the final conv's operand: the LSTM
    // output as two fp16 pieces in windowed layout [2][B][32][Lpf][16] (6 reflected front rows, output rows padded to 256 per clip)
    p.Mpf = ((int)T + 255) / 256 * 256;
    p.Lpf = p.Mpf + 8;
    const size_t xs_lstm = (((size_t)B * T + 255) / 256 * 256) * kH * 3 / 2, xs_fin = (size_t)B * p.Lpf * kH + 64;
    p.off_xs = take(xs_lstm > xs_fin ? xs_lstm : xs_fin);
    p.total_floats = cur;
    return p;
}

// Streaming encode (at_encodec_encode_stream_checked). State of B streams, floats: the last kStreamCtx consumed samples [B][640], h and c of
// the two LSTM layers [4][B][512] (h0, c0, h1, c1), the last kStreamHist rows of ELU(lstm + skip) [B][6][512] (the final conv's history).
// A frame of the LSTM's input depends on samples back to 320 t - 478 (conv0 6, four blocks 2 each at their rate, strided convs 2, 4, 5, 8), so two
// frames are the smallest frame-aligned context; the first two output frames of a window [context | new] are dropped.
constexpr int kHop = 320, kStreamCtx = 2 * kHop, kStreamDrop = 2, kStreamHist = 6;
constexpr int kFinPad = 6;              // reflected front rows of the final k = 7 conv; a clip of <= 6 frames is zero-extended to 7 rows first (the reference's rule)
constexpr int kStreamFirstFrames = 7;  // a stream's first push (unless final) fills the final conv's history and takes its reflected front rows from real rows
struct StreamState {
    float *ctx, *h[2], *c[2], *yhist;
    StreamState(void* base, int B) {
        ctx = yhist = h[0] = h[1] = c[0] = c[1] = nullptr;
        if (!base) return;
        float* f = (float*)base;
        ctx = f; f += (size_t)B * kStreamCtx;
        for (int l = 0; l < 2; ++l) { h[l] = f; f += (size_t)B * kH; c[l] = f; f += (size_t)B * kH; }
        yhist = f;
    }
    static size_t floats(int B) { return (size_t)B * (kStreamCtx + 4 * kH + kStreamHist * kH); }
};
struct StreamCall { const void* state_in; void* state_out; bool started, final; };
// The window's plan plus the mid-stream buffers. They live where the plan has room at that moment: the window itself in the (not yet
// written) gate buffer, everything behind the conv stack in the stage buffers the conv stack has finished with; only when those are too small
// (a tiny "subbatch" against a large B) behind the plan. So a push needs no more workspace than a one-shot encode of its window.
struct StreamPlan {
    EncPlan p;
    int Tn = 0, Ty = 0, Mpf = 0, Lpf = 0;   // new frames; rows / padded rows / operand rows of the final conv's input [history | new]
    size_t off_win = 0, off_x4n = 0, off_yw = 0, off_embw = 0, off_yp = 0, off_emb = 0;
    size_t total_floats = 0;
};
inline StreamPlan make_stream_plan(int B, int n_new, bool started, int sub) {
    StreamPlan sp;
    sp.p = make_plan(B, n_new + (started ? kStreamCtx : 0), sub);
    sp.total_floats = sp.p.total_floats;
    sp.Tn = sp.p.L[4] - (started ? kStreamDrop : 0);
    if (!started) return sp;
    sp.Ty = sp.Tn + kStreamHist;
    sp.Mpf = (sp.Ty + 255) / 256 * 256;
    sp.Lpf = sp.Mpf + 8;
    sp.off_win = sp.p.off_xg;   // B * (640 + n_new) floats <= B * T * 2048
    size_t cur = 0;
    auto take = [&](size_t n) { size_t o = cur; cur += (n + 63) / 64 * 64; return o; };
    sp.off_x4n = take((size_t)B * sp.Tn * kH);
    sp.off_yw = take((size_t)B * sp.Ty * kH);
    sp.off_embw = take((size_t)B * sp.Ty * kDim);
    sp.off_yp = take((size_t)B * sp.Lpf * kH + 64);
    sp.off_emb = take((size_t)B * sp.Tn * kDim);
    if (cur > sp.p.off_x4) {   // does not fit the finished stage buffers: behind the plan
        const size_t base = sp.p.total_floats;
        sp.off_x4n += base; sp.off_yw += base; sp.off_embw += base; sp.off_yp += base; sp.off_emb += base;
        sp.total_floats += cur;
    }
    return sp;
}

struct DecPlan {
    int L[5];  // L[0] = T, L[s+1] = L[s]*ratio
    int G;
    size_t off_z, off_x0, off_xg, off_xg2, off_h0, off_h1, off_c, off_y, off_sync, off_xs;
    size_t off_u[4], off_h[4], off_r[4];
    size_t off_ap;     // operand pieces of a transposed conv run as a windowed split GEMM: [2][G][Cin/16][Lpu][16] fp16 (one float per element)
    int dMpc = 0, dLpc = 0; size_t off_dac3 = 0, off_dat3 = 0;   // stage-0 block as split GEMMs: padded rows, k3 operand [2][G][16][dLpc][16], tail operand [2][G][24][dMpc][16]
    int Mpu[3], Lpu[3];   // per stage: padded output rows / operand rows per clip
    size_t total_floats;
};

inline DecPlan make_dec_plan(int B, int T, int sub) {
    DecPlan p;
    p.L[0] = T;
    for (int s = 0; s < 4; ++s) p.L[s + 1] = p.L[s] * kRatiosDec[s];
    p.G = B < sub ? B : sub;
    size_t cur = 0;
    auto take = [&](size_t n) { size_t o = cur; cur += (n + 63) / 64 * 64; return o; };
    p.off_z = take((size_t)B * T * kDim);
    p.off_x0 = take((size_t)B * T * kH);
    p.off_xg = take((size_t)B * T * 4 * kH);
    p.off_xg2 = take(B <= kPipeMaxClips ? (size_t)B * T * 4 * kH : 0);
    p.off_h0 = take((size_t)B * T * kH);
    p.off_h1 = take((size_t)B * T * kH);
    p.off_c = take((size_t)B * kH);
    p.off_y = take((size_t)B * T * kH);
    p.off_sync = take(1024);
    p.off_xs = take((((size_t)B * T + 255) / 256 * 256) * kH * 3 / 2);   // split-bf16 copy of an LSTM layer's input
    int C = kH;
    for (int s = 0; s < 4; ++s) {
        C /= 2;
        p.off_u[s] = take((size_t)p.G * p.L[s + 1] * C);
        p.off_h[s] = take((size_t)p.G * p.L[s + 1] * (C / 2));
        p.off_r[s] = take((size_t)p.G * p.L[s + 1] * C);
    }
    {
        size_t ap = 0;
        int Cin = kH;
        for (int s = 0; s < 3; ++s) {
            p.Mpu[s] = (p.L[s] + 255) / 256 * 256;
            p.Lpu[s] = p.Mpu[s] + 8;
            const size_t n = (size_t)p.G * Cin * p.Lpu[s];
            ap = n > ap ? n : ap;
            Cin /= 2;
        }
        p.off_ap = take(ap + 64);
    }
    p.dMpc = (p.L[1] + 255) / 256 * 256;
    p.dLpc = (p.dMpc + 2 + 63) / 64 * 64;
    p.off_dac3 = take((size_t)p.G * p.dLpc * 256 + 64);
    p.off_dat3 = take((size_t)p.G * p.dMpc * 384 + 64);
    p.total_floats = cur;
    return p;
}

// Streaming decode (at_encodec_decode_stream_checked). State of B streams, floats: the last kDecHist rows of the quantised embedding z [B][6][128]
// (the history of the k = 7 first conv), h and c of the two LSTM layers [4][B][512] (h0, c0, h1, c1), the last kDecCtx rows of ELU(lstm + skip)
// [B][2][512]. An output sample n reaches back to row floor(n / 320) - 2 of that tensor (final conv 6 samples, per stage the block's k3 conv 2 rows
// and the transposed conv 1 input row), so the upsampling stack runs on [2 carried rows | new rows] and its first 640 samples are never stored.
constexpr int kDecHist = 6, kDecCtx = 2, kDecFirstFrames = 7;
struct DecStreamState {
    float *zhist, *h[2], *c[2], *yctx;
    DecStreamState(void* base, int B) {
        zhist = yctx = h[0] = h[1] = c[0] = c[1] = nullptr;
        if (!base) return;
        float* f = (float*)base;
        zhist = f; f += (size_t)B * kDecHist * kDim;
        for (int l = 0; l < 2; ++l) { h[l] = f; f += (size_t)B * kH; c[l] = f; f += (size_t)B * kH; }
        yctx = f;
    }
    static size_t floats(int B) { return (size_t)B * (kDecHist * kDim + 4 * kH + kDecCtx * kH); }
};
struct DecStreamCall { const void* state_in; void* state_out; bool started; };
// The one-shot plan of the window (Tw = new + context rows; the LSTM buffers hold the new rows only) and, behind it, the two windows the state
// kernel writes: z [B][Tz][128] and ELU(lstm + skip) [B][Tw][512].
struct DecStreamPlan {
    DecPlan p;
    int Tz = 0, Tw = 0;
    size_t off_zw = 0, off_yw = 0, total_floats = 0;
};
inline DecStreamPlan make_dec_stream_plan(int B, int t_new, bool started, int sub) {
    DecStreamPlan sp;
    sp.Tz = t_new + (started ? kDecHist : 0);
    sp.Tw = t_new + (started ? kDecCtx : 0);
    sp.p = make_dec_plan(B, sp.Tw, sub);
    size_t cur = sp.p.total_floats;
    auto take = [&](size_t n) { size_t o = cur; cur += (n + 63) / 64 * 64; return o; };
    sp.off_zw = take((size_t)B * sp.Tz * kDim);
    sp.off_yw = take((size_t)B * sp.Tw * kH);
    sp.total_floats = cur;
    return sp;
}

// ---- routes ----------------------------------------------------------------------------------------------------------------------------------
// Which split weights finalize() made (all of them with bf16x3, none without; the decoder's only with a decoder): the routes ask for the weight
// a kernel needs, not for the switch that made it.
struct EncHave { bool down2_s, down3_s, res3c_s, chain_f0, fin_f; };
struct DecHave { bool dchain_f[2], dup_f[3], dres_fs[4], dtail_up_fs; };

// kernel of a 64- / 128-channel residual block (RES_GEMM: the block as two fp32 windowed GEMMs, any width)
enum ResKernel { RES_GEMM, RES64, RES64_X3, RES128, RES128_X3, RES128_RS };
inline ResKernel res64_kernel(const Options& o, bool bf16x3) { return !o.fused_res64 ? RES_GEMM : (o.res64_x3 && bf16x3) ? RES64_X3 : RES64; }
inline ResKernel res128_kernel(const Options& o, bool bf16x3, bool f16) {
    if (!o.fused_res128) return RES_GEMM;
    const bool x3 = o.res128_x3 && bf16x3;
    return (x3 && o.res128_rs && f16) ? RES128_RS : x3 ? RES128_X3 : RES128;
}

// The encoder's conv stack and final conv. L[0..4] = the plan's lengths in front of each stage; every sub-batch of a call takes the same route.
struct EncRoute {
    bool fused0;         // stage 0 in one kernel (else conv0 + GEMM block + fp32 strided conv)
    bool stage1_fused;   // stage 1 in one kernel (seanet_res64down.hip); else res1 + down64
    ResKernel res1;
    bool down64;         // stage-1 strided conv: seanet_down64* (else the fp32 windowed GEMM)
    ResKernel res2;
    bool down2_gemm;     // the 128-channel block writes split pieces, the stage-2 strided conv is a split GEMM
    bool chain3;         // stage-2 strided conv -> 256-channel block -> stage-3 strided conv as chained split GEMMs (no fp32 in between)
    bool down3_gemm;     // stage-3 strided conv as a split GEMM; without chain3 a stand-alone pass splits its input first
    bool cf;             // operand scheme of that chain: two fp16 pieces / three products (default) or three bf16 pieces / six products
    int cnp;             // its pieces per operand
    enum Fin { FIN_SHORT, FIN_F16X2, FIN_F32 } fin;   // FIN_SHORT: fewer rows than the k = 7 conv reflects (one-shot clips of 321..1920 samples; mid-stream Ty >= 7)
};
inline EncRoute enc_route(const Options& o, bool bf16x3, const EncHave& w, const EncPlan& p, int Ty) {
    const int* L = p.L;
    EncRoute r;
    r.fused0 = o.fused_stage0 && L[0] % 2 == 0;
    // stage 1 in one kernel: the block output (the largest tensor of the path) stays in LDS
    r.stage1_fused = o.fused_stage1 && o.fused_res64 && o.fused_down64 && bf16x3 && o.res64_x3 && o.down64_x3 && o.res_f16x2 && L[1] % 4 == 0 && L[1] >= 8;
    r.res1 = res64_kernel(o, bf16x3);
    r.down64 = o.fused_down64 && L[1] % 4 == 0;
    r.res2 = res128_kernel(o, bf16x3, o.res_f16x2);
    // with the strided conv as a split-bf16 GEMM the block writes that GEMM's operand pieces instead of fp32 rows
    r.down2_gemm = r.res2 != RES_GEMM && o.down128_x3 && o.res128_x3 && bf16x3 && w.down2_s && L[2] % 5 == 0 && L[2] >= 10;
    r.chain3 = r.down2_gemm && o.res256_x3 && o.down256_x3 && w.res3c_s && w.down3_s && L[3] % 8 == 0 && L[3] >= 16;
    r.down3_gemm = o.down256_x3 && bf16x3 && w.down3_s && L[3] % 8 == 0 && L[3] >= 16;
    r.cf = o.chain_f16x2 && w.chain_f0;
    r.cnp = r.cf ? 2 : 3;
    r.fin = Ty <= kFinPad ? EncRoute::FIN_SHORT : (bf16x3 && o.fin_f16x2 && w.fin_f) ? EncRoute::FIN_F16X2 : EncRoute::FIN_F32;
    return r;
}

// The decoder's upsampling stack. Stage s: transposed conv (Cin = 512 >> s -> Co = Cin / 2, L[s] -> L[s + 1] rows) + the Co-channel block.
struct DecRoute {
    enum Tail { TAIL_CONV_LAST, TAIL_FUSED, TAIL_FUSED_X2 } tail;   // stage 3 + final conv in one kernel (fp32 / fp16 scheme), or stage 3 as the others + conv_last
    bool up_gemm[4];     // the transposed conv as a two-tap windowed split GEMM on the fp16 scheme (else the fp32 GEMM)
    bool chain0;         // stage-0 block as split GEMMs whose tail writes stage 1's transposed-conv operand: stage 1 runs no split pass
    ResKernel res[4];    // blocks of the stages that do not run chained / in the tail kernel
    bool res_f16[4];     // ... with their own contractions on the two-piece fp16 scheme
};
inline DecRoute dec_route(const Options& o, bool bf16x3, const DecHave& w, const DecPlan& p) {
    const int* L = p.L;
    DecRoute r;
    r.tail = !(o.fused_dectail && L[3] >= 8) ? DecRoute::TAIL_CONV_LAST
             : (o.tail_f16x2 && bf16x3 && w.dtail_up_fs && w.dres_fs[3]) ? DecRoute::TAIL_FUSED_X2 : DecRoute::TAIL_FUSED;
    for (int s = 0; s < 4; ++s) {
        r.up_gemm[s] = s < 3 && bf16x3 && o.up_f16x2 && w.dup_f[s] && L[s] > 1;
        r.res_f16[s] = o.res_f16x2 && w.dres_fs[s];
        r.res[s] = s == 1 ? res128_kernel(o, bf16x3, r.res_f16[s]) : s == 2 ? res64_kernel(o, bf16x3) : RES_GEMM;   // 256, 128, 64, 32 channels
    }
    r.chain0 = o.dec_chain && bf16x3 && o.res_f16x2 && o.up_f16x2 && w.dchain_f[0] && w.dchain_f[1] && w.dup_f[1] && L[1] >= 3;
    return r;
}

// The 2-layer LSTM of either side. The rules, all of them: the fp16-scheme input projection needs bf16x3 (finalize makes the operand pieces with it); the
// matrix-core recurrence needs bf16x3 and "lstm_x3"; small batches take both layers in one pipelined launch after layer 1's projection (lstm_pipe.hip:
// same arithmetic, ~half the dependent steps) when every part of it is on the fp16 scheme and the device agrees (pipe_fits = lstm_pipe_eligible(B, T)); and
// a carried state (streaming) with the three-piece bf16 recurrence, which has no state variant (lstm_seq_x3.hip), runs the fp32 persistent kernel.
struct LstmRoute {
    enum Ih { IH_F16X2, IH_BF16X3, IH_F32 } ih;                                             // input projections
    enum Rec { REC_PIPE, REC_SEQ_F16X2, REC_SEQ_BF16X3, REC_SEQ_F32, REC_STEPWISE } rec;   // recurrence
};
inline LstmRoute lstm_route(const Options& o, bool bf16x3, int B, bool pipe_fits, bool carry) {
    LstmRoute r;
    r.ih = (bf16x3 && o.ih_f16x2) ? LstmRoute::IH_F16X2 : bf16x3 ? LstmRoute::IH_BF16X3 : LstmRoute::IH_F32;
    const bool x3 = bf16x3 && o.lstm_x3;
    if (!o.persistent_lstm) r.rec = LstmRoute::REC_STEPWISE;
    else if (x3 && o.lstm_f16x2)
        r.rec = (r.ih == LstmRoute::IH_F16X2 && o.lstm_pipe && B <= kPipeMaxClips && pipe_fits) ? LstmRoute::REC_PIPE : LstmRoute::REC_SEQ_F16X2;
    else r.rec = (x3 && !carry) ? LstmRoute::REC_SEQ_BF16X3 : LstmRoute::REC_SEQ_F32;
    return r;
}

}  // namespace at
