// Acoustic tokenizer: what the encode and the decode side share. The fp32 conv / residual-block building blocks, and the 2-layer LSTM + skip, run by
// the kernels that lstm_route (encodec_plan.h) names.
#include "encodec_handle.h"

namespace at {

// ---- building blocks the encode and the decode side share ----------------------------------------------------------------------------------
// One causal conv as a windowed GEMM over `batch` clips.
int conv_gemm(const ConvW& c, const float* X, long long x_bstride, int Tin, float* C, long long c_bstride, int M, int batch,
              int pro, const float* R, long long r_bstride, hipStream_t stream, int pad_mode, int epi) {
    GemmArgs a;
    a.X = X; a.x_bstride = x_bstride; a.Tin = Tin; a.Cin = c.cin; a.ldx = c.cin;
    a.ktaps = c.k; a.stride = c.stride; a.pad_left = c.k - c.stride; a.pad_mode = pad_mode;
    a.W = c.w; a.bias = c.b;
    a.C = C; a.c_bstride = c_bstride; a.ldc = c.cout;
    a.R = R; a.r_bstride = r_bstride; a.ldr = c.cout;
    a.M = M; a.N = c.cout; a.K = c.k * c.cin; a.batch = batch;
    a.pro = pro; a.epi = epi; a.alpha = 1.0f;
    return launch_gemm(a, stream);
}

// SEANet residual block: out = shortcut(x) + conv1(ELU(conv3(ELU(x)))) as TWO windowed GEMMs:
//   h   = ELU(conv3(ELU(x)))                             K = 3C,  N = C/2   (the inner ELU once per element, in the epilogue)
//   out = [h | x] . [W1 | Wsc]^T + (b1 + bsc)            K = C/2 + C, N = C   (dual-source A, weights concatenated
// at finalize) — one pass less over the block output than "shortcut, then accumulate".
int resblock(const ConvW (&r)[3], const float* x, float* hbuf, float* out, int L, int batch, hipStream_t stream, int epi) {
    const int C = r[2].cout;
    const long long xs = (long long)L * C, hs = (long long)L * (C / 2);
    if (int rc = conv_gemm(r[0], x, xs, L, hbuf, hs, L, batch, PRO_ELU, nullptr, 0, stream, 1, EPI_ELU)) return rc;
    GemmArgs a;
    a.X = hbuf; a.x_bstride = hs; a.Tin = L; a.Cin = C / 2; a.ldx = C / 2;
    a.X2 = x; a.x2_bstride = xs; a.ld2 = C; a.K1 = C / 2;
    a.W = r[1].w; a.bias = r[1].b;     // r[1] holds the concatenated [C][C/2 + C] weight and the summed bias
    a.C = out; a.c_bstride = xs; a.ldc = C;
    a.M = L; a.N = C; a.K = C / 2 + C; a.batch = batch; a.pro = PRO_NONE; a.epi = epi;
    return launch_gemm(a, stream);
}

int launch_res_kernel(ResKernel k, const Res64Args& ra, hipStream_t stream) {
    switch (k) {
        case RES64: return launch_seanet_res64(ra, stream);
        case RES64_X3: return launch_seanet_res64x3(ra, stream);
        case RES128: return launch_seanet_res128(ra, stream);
        case RES128_X3: return launch_seanet_res128x3(ra, stream);
        case RES128_RS: return launch_seanet_res128rs(ra, stream);
        default: set_error("launch_res_kernel: not a fused block"); return -1;
    }
}

// ---- the LSTM --------------------------------------------------------------------------------------------------------------------------------
namespace {

// layer's input gates xg = in . W_ih^T + b_ih over all B * T rows
int lstm_input_gates(const LstmW& w, int layer, const float* in, const LstmBufs& b, int B, int T, LstmRoute::Ih ih, int* range_status, hipStream_t stream) {
    const long long M = (long long)B * T, Mpad = (M + 255) / 256 * 256;
    if (ih == LstmRoute::IH_F32) {
        GemmArgs g;
        g.X = in; g.x_bstride = 0; g.Tin = B * T; g.Cin = kH; g.ldx = kH;
        g.W = w.wih[layer]; g.bias = w.bih[layer];
        g.C = b.xg; g.ldc = 4 * kH; g.M = B * T; g.N = 4 * kH; g.K = kH; g.batch = 1;
        return launch_gemm(g, stream);
    }
    Bf16x3Args a;
    a.A = b.xs; a.bias = w.bih[layer]; a.M = (int)M; a.N = 4 * kH; a.K = kH; a.Mpad = (int)Mpad;
    a.epi = XB_EPI_LINEAR; a.C = b.xg; a.ldc = 4 * kH; a.alpha = 1.0f;
    if (ih == LstmRoute::IH_F16X2) {   // two fp16 pieces per operand, three MFMA products (gemm_f16x2_tg.hip for full batches)
        if (int rc = launch_split_blocked(in, kH, M, Mpad, kH, b.xs, stream, XB_SCHEME_F16X2, XB_F16_ACT_SCALE, range_status)) return rc;
        use_f16x2(a, SplitW{w.wih_f[layer], w.wih_fs[layer]}, range_status);
    } else {   // split-bf16 GEMM (gemm_bf16x3.hip): x -> 3 bf16 pieces, then 6 bf16 MFMAs per step
        if (int rc = launch_split_blocked(in, kH, M, Mpad, kH, b.xs, stream)) return rc;
        a.W = w.wih_s[layer];
    }
    return launch_gemm_bf16x3(a, stream);
}

// one layer, one launch per time step (no persistent kernel on this device, or $AUDIOTOKEN_LSTM_STEPWISE)
int lstm_stepwise(const LstmW& w, int layer, const LstmBufs& b, float* hout, int B, int T, const LstmCarry* carry, hipStream_t stream) {
    if (carry) AT_CHECK_HIP(hipMemcpyAsync(b.c, carry->c_init[layer], (size_t)B * kH * sizeof(float), hipMemcpyDeviceToDevice, stream));
    for (int t = 0; t < T; ++t) {
        GemmArgs s;
        s.X = hout + (long long)(t > 0 ? t - 1 : 0) * kH; s.x_bstride = 0; s.Tin = B; s.Cin = kH; s.ldx = T * kH;
        if (carry && t == 0) { s.X = carry->h_init[layer]; s.ldx = kH; }   // h_{-1} = the carried h, [B][512]
        s.W = w.whh[layer]; s.M = B; s.N = 4 * kH; s.K = kH; s.batch = 1; s.ldc = 4 * kH;
        LstmStepArgs ls;
        ls.xg = b.xg; ls.b_hh = w.bhh[layer]; ls.c = b.c; ls.h_out = hout;
        ls.y_out = layer == 1 ? b.y : nullptr; ls.skip = b.x;
        ls.T = T; ls.t = t; ls.H = kH; ls.first = t == 0 && !carry; ls.y_elu = 1;
        if (int rc = launch_lstm_step(s, ls, stream)) return rc;
    }
    if (carry) AT_CHECK_HIP(hipMemcpyAsync(carry->c_final[layer], b.c, (size_t)B * kH * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

}  // namespace

// Carried state (streaming): every route starts layer l from (h_init[l], c_init[l]) and leaves its last cell state in c_final[l]; the last
// h is row T - 1 of h0 / h1.
int lstm_skip(at_encodec* h, const LstmW& w, const LstmBufs& b, int B, int T, const LstmCarry* carry, LstmRoute route, int* range_status, hipStream_t stream) {
    Profiler& prof = h->prof;
    for (int layer = 0; layer < 2; ++layer) {
        float* hout = layer == 0 ? b.h0 : b.h1;
        prof.begin("lstm_ih", 1, stream);
        if (int rc = lstm_input_gates(w, layer, layer == 0 ? b.x : b.h0, b, B, T, route.ih, range_status, stream)) return rc;
        prof.end(stream);
        if (route.rec == LstmRoute::REC_PIPE) {
            LstmPipeArgs q;
            q.xg1 = b.xg; q.w_hh1 = w.whh[0]; q.b_hh1 = w.bhh[0]; q.w_ih2 = w.wih[1]; q.b_ih2 = w.bih[1]; q.w_hh2 = w.whh[1]; q.b_hh2 = w.bhh[1];
            q.h1 = b.h0; q.xg2 = b.xg2; q.h2 = b.h1; q.y_out = b.y; q.skip = b.x; q.sync = b.sync; q.B = B; q.T = T; q.y_elu = 1; q.spin_limit = h->lstm_spin_limit;
            q.ws_hh1 = w.whh_fs[0]; q.ws_ih2 = w.wih_fs[1]; q.ws_hh2 = w.whh_fs[1]; q.act_scale = XB_F16_ACT_SCALE;
            if (carry)
                for (int l = 0; l < 2; ++l) { q.h_init[l] = carry->h_init[l]; q.c_init[l] = carry->c_init[l]; q.c_final[l] = carry->c_final[l]; }
            prof.begin("lstm_rec", 1, stream);
            if (int rc = launch_lstm_pipe(q, stream)) return rc;
            prof.end(stream);
            return 0;
        }
        if (route.rec == LstmRoute::REC_STEPWISE) {
            prof.begin("lstm_rec", T, stream);
            if (int rc = lstm_stepwise(w, layer, b, hout, B, T, carry, stream)) return rc;
            prof.end(stream);
            continue;
        }
        // whole sequence in one persistent launch per 256-clip block (lstm_seq.hip)
        const bool x3 = route.rec != LstmRoute::REC_SEQ_F32;
        const int maxc = x3 ? lstm_seq_x3_max_clips() : lstm_seq_max_clips();
        prof.begin("lstm_rec", (B + maxc - 1) / maxc, stream);
        for (int c0 = 0; c0 < B; c0 += maxc) {
            LstmSeqArgs q;
            const long long ro = (long long)c0 * T;
            q.xg = b.xg + ro * 4 * kH; q.w_hh = w.whh[layer]; q.b_hh = w.bhh[layer]; q.h_out = hout + ro * kH;
            q.y_out = layer == 1 ? b.y + ro * kH : nullptr; q.skip = b.x + ro * kH; q.sync = b.sync;
            q.B = (B - c0) < maxc ? (B - c0) : maxc; q.T = T; q.n_groups = 0; q.h_bytes = 0; q.y_elu = 1; q.spin_limit = h->lstm_spin_limit;
            q.w_scale_f16 = route.rec == LstmRoute::REC_SEQ_F16X2 ? w.whh_fs[layer] : 0.f;
            if (carry) { q.h_init = carry->h_init[layer] + (long long)c0 * kH; q.c_init = carry->c_init[layer] + (long long)c0 * kH; q.c_final = carry->c_final[layer] + (long long)c0 * kH; }
            if (int rc = x3 ? launch_lstm_seq_x3(q, stream) : launch_lstm_seq(q, stream)) return rc;
        }
        prof.end(stream);
    }
    return 0;
}

}  // namespace at
