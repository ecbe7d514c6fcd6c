// Acoustic tokenizer, encode side: waveform -> SEANet conv stack (per sub-batch) -> LSTM -> final conv -> RVQ search, one-shot or as one push of a
// stream. The kernels of a call are chosen once, by enc_route / lstm_route (encodec_plan.h); the stage functions below launch them.
// Replaces reference AcousticEncoder (audiotoken/encoder.py:29-57), whose arithmetic is the PyPI `encodec` model; architecture per SURVEY.md Appendix A.1.
#include "encodec_handle.h"

namespace at {

namespace {

const char* const kRes[4] = {"res0", "res1", "res2", "res3"};
const char* const kDown[4] = {"down0", "down1", "down2", "down3"};

// the block of stage s as two fp32 GEMMs, its output r[s] already through the ELU of the strided conv that alone consumes it
int enc_gemm_block(at_encodec* h, const EncPlan& p, float* ws, int s, int g, hipStream_t stream) {
    h->prof.begin(kRes[s], 2, stream);
    if (int rc = resblock(h->res[s], ws + p.off_x[s], ws + p.off_h[s], ws + p.off_r[s], p.L[s], g, stream, EPI_ELU)) return rc;
    h->prof.end(stream);
    return 0;
}
// the strided conv of stage s as an fp32 windowed GEMM, r[s] -> out
int enc_gemm_down(at_encodec* h, const EncPlan& p, float* ws, int s, float* out, int g, hipStream_t stream) {
    const int C = 32 << s, L = p.L[s], Lo = p.L[s + 1];
    return conv_gemm(h->down[s], ws + p.off_r[s], (long long)L * C, L, out, (long long)Lo * 2 * C, Lo, g, PRO_NONE, nullptr, 0, stream);
}
void res_args(const at_encodec* h, int s, const float* x, float* out, int g, int L, int site, Res64Args& ra) {
    ra.x = x; ra.out = out; ra.w3 = h->res[s][0].w; ra.b3 = h->res[s][0].b; ra.wt = h->res[s][1].w; ra.bt = h->res[s][1].b;
    ra.B = g; ra.L = L;
    if (h->opt.res_f16x2) { ra.scheme = XB_SCHEME_F16X2; ra.act_scale = XB_F16_ACT_SCALE; ra.w3_scale = h->res_fs[s][0]; ra.wt_scale = h->res_fs[s][1]; ra.status = range_site(h, site); }
}

// waveform -> x[1] (fused) or x[0] -> r[0] -> x[1]
int enc_stage0(at_encodec* h, const EncRoute& r, const EncPlan& p, float* ws, const float* wav, int g, hipStream_t stream) {
    Profiler& prof = h->prof;
    const int N = p.L[0];
    if (!r.fused0) {
        prof.begin("conv0", 1, stream);
        if (int rc = launch_conv0(wav, h->conv0.w, h->conv0.b, ws + p.off_x[0], g, N, stream)) return rc;
        prof.end(stream);
        if (int rc = enc_gemm_block(h, p, ws, 0, g, stream)) return rc;
        prof.begin(kDown[0], 1, stream);
        if (int rc = enc_gemm_down(h, p, ws, 0, ws + p.off_x[1], g, stream)) return rc;
        prof.end(stream);
        return 0;
    }
    // conv0 + resblock(32) + ELU + strided conv in one kernel: 4 B in, 128 B out per sample (seanet_stage0.hip)
    Stage0Args sa;
    sa.wav = wav; sa.x1 = ws + p.off_x[1];
    sa.w0 = h->conv0.w; sa.b0 = h->conv0.b; sa.w3 = h->res[0][0].w; sa.b3 = h->res[0][0].b;
    sa.wt = h->res[0][1].w; sa.bt = h->res[0][1].b; sa.wd = h->down[0].w; sa.bd = h->down[0].b;
    sa.B = g; sa.N = N;
    sa.wsc0 = h->sc0_w; sa.bsc0 = h->sc0_w ? h->sc0_w + 32 * 7 : nullptr;
    if (h->opt.res_f16x2) {
        sa.scheme = XB_SCHEME_F16X2; sa.act_scale = XB_F16_ACT_SCALE; sa.status = range_site(h, AS_STAGE0);
        sa.w3_scale = h->res_fs[0][0]; sa.wt_scale = h->res_fs[0][1]; sa.wd_scale = h->down_fs[0];
    }
    prof.begin("stage0_fused", 1, stream);
    if (int rc = (h->opt.stage0_x3 && h->bf16x3) ? launch_seanet_stage0x3(sa, stream) : launch_seanet_stage0(sa, stream)) return rc;
    prof.end(stream);
    return 0;
}

// x[1] -> x[2]
int enc_stage1(at_encodec* h, const EncRoute& r, const EncPlan& p, float* ws, int g, hipStream_t stream) {
    Profiler& prof = h->prof;
    const int L = p.L[1];
    float *x = ws + p.off_x[1], *rb = ws + p.off_r[1], *out = ws + p.off_x[2];
    if (r.stage1_fused) {
        ResDown64Args fa;
        fa.x = x; fa.out = out; fa.w3 = h->res[1][0].w; fa.b3 = h->res[1][0].b; fa.wt = h->res[1][1].w; fa.bt = h->res[1][1].b;
        fa.wd = h->down[1].w; fa.bd = h->down[1].b; fa.B = g; fa.L = L;
        fa.act_scale = XB_F16_ACT_SCALE; fa.w3_scale = h->res_fs[1][0]; fa.wt_scale = h->res_fs[1][1]; fa.wd_scale = h->down_fs[1];
        fa.status_res = range_site(h, AS_RES1); fa.status_down = range_site(h, AS_DOWN1);
        prof.begin("res1_down1", 1, stream);
        if (int rc = launch_seanet_res64down(fa, stream)) return rc;
        prof.end(stream);
        return 0;
    }
    if (r.res1 == RES_GEMM) {
        if (int rc = enc_gemm_block(h, p, ws, 1, g, stream)) return rc;
    } else {
        // 64-channel block fused into one kernel: 256 B in + 256 B out per row (seanet_res64.hip)
        Res64Args ra;
        res_args(h, 1, x, rb, g, L, AS_RES1, ra);
        prof.begin("res1", 1, stream);
        if (int rc = launch_res_kernel(r.res1, ra, stream)) return rc;
        prof.end(stream);
    }
    prof.begin(kDown[1], 1, stream);
    if (r.down64) {
        Down64Args da;
        da.x = rb; da.out = out; da.w = h->down[1].w; da.b = h->down[1].b; da.B = g; da.L = L;
        if (h->opt.res_f16x2) { da.scheme = XB_SCHEME_F16X2; da.act_scale = XB_F16_ACT_SCALE; da.w_scale = h->down_fs[1]; da.status = range_site(h, AS_DOWN1); }
        if (int rc = (h->opt.down64_x3 && h->bf16x3) ? launch_seanet_down64x3(da, stream) : launch_seanet_down64(da, stream)) return rc;
    } else if (int rc = enc_gemm_down(h, p, ws, 1, out, g, stream)) {
        return rc;
    }
    prof.end(stream);
    return 0;
}

// weight and scheme of GEMM j of the stage 2-3 chain: 0 = stage-2 strided conv, 1 = conv3 of the 256-channel block, 2 = its tail, 3 = stage-3 conv
void chain_cfg(const at_encodec* h, const EncRoute& r, Bf16x3Args& a, int j, const __bf16* w_bf16) {
    if (r.cf) use_f16x2(a, h->chain_f[j], range_site(h, j == 0 ? AS_DOWN2 : j == 1 ? AS_RES3_CONV : AS_RES3_TAIL));
    else a.W = w_bf16;
}

// x[2] -> x[3] as fp32 rows, or (chain3) as the operand pieces of the 256-channel block
int enc_stage2(at_encodec* h, const EncRoute& r, const EncPlan& p, float* ws, int g, hipStream_t stream) {
    Profiler& prof = h->prof;
    const int L = p.L[2], Lo = p.L[3];
    float *x = ws + p.off_x[2], *rb = ws + p.off_r[2], *out = ws + p.off_x[3];
    if (r.res2 == RES_GEMM) {
        if (int rc = enc_gemm_block(h, p, ws, 2, g, stream)) return rc;
    } else {
        // 128-channel block fused: weights stationary in registers, h never leaves the CU (seanet_res128.hip)
        Res64Args ra;
        res_args(h, 2, x, rb, g, L, AS_RES2, ra);
        if (r.down2_gemm) {   // the block writes the strided conv's operand pieces instead of fp32 rows
            ra.S = reinterpret_cast<__bf16*>(rb); ra.Lp = p.Lp2;
            if (r.cf) { ra.S_scheme = XB_SCHEME_F16X2; ra.S_scale = XB_F16_ACT_SCALE; ra.status = range_site(h, AS_RES2); }
        }
        prof.begin("res2", r.down2_gemm ? 2 : 1, stream);
        if (int rc = launch_res_kernel(r.res2, ra, stream)) return rc;
        if (r.down2_gemm)
            if (int rc = launch_reflect_front5(ra.S, g, 8, p.Lp2, stream, r.cnp)) return rc;
        prof.end(stream);
    }
    prof.begin(kDown[2], 1, stream);
    if (r.down2_gemm) {
        Bf16x3Args ga;
        ga.A = reinterpret_cast<const __bf16*>(rb); chain_cfg(h, r, ga, 0, h->down2_s); ga.bias = h->down[2].b;
        ga.M = Lo; ga.Mpad = p.Mp2; ga.N = 256; ga.K = 1280;
        ga.batch = g; ga.stride = 5; ga.cblocks = 8; ga.Lp = p.Lp2;
        if (r.chain3) {   // the next block reads pieces: raw x -> K-blocks 8..23 of its tail operand, ELU(x) (2 causal front rows) -> its conv3 operand
            ga.epi = XB_EPI_RAW_ELU_SPLIT2;
            ga.S = reinterpret_cast<__bf16*>(ws + p.off_at3); ga.Spad = p.Mpc; ga.Sphases = 1; ga.Sfront = 0; ga.Sblocks = 24; ga.Sblock0 = 8;
            ga.S2 = reinterpret_cast<__bf16*>(ws + p.off_ac3); ga.S2pad = p.Lpc; ga.S2phases = 1; ga.S2front = 2;
        } else {
            ga.epi = XB_EPI_LINEAR; ga.C = out; ga.ldc = 256;
        }
        if (int rc = launch_gemm_bf16x3(ga, stream)) return rc;
        if (r.chain3)
            if (int rc = launch_reflect_front(ga.S2, g, 16, 1, p.Lpc, 2, stream, r.cnp)) return rc;
    } else if (int rc = enc_gemm_down(h, p, ws, 2, out, g, stream)) {
        return rc;
    }
    prof.end(stream);
    return 0;
}

// x[3] (or the chain's pieces) -> this sub-batch's rows of the LSTM input
int enc_stage3(at_encodec* h, const EncRoute& r, const EncPlan& p, float* ws, float* out, int g, hipStream_t stream) {
    Profiler& prof = h->prof;
    const int L = p.L[3], Lo = p.L[4];
    __bf16* s3 = reinterpret_cast<__bf16*>(ws + p.off_s3);
    if (r.chain3) {
        // conv3 (k3, 256 -> 128) on the ELU pieces the stage-2 GEMM wrote; its ELU_SPLIT epilogue fills K-blocks 0..7 of the tail's
        // operand (blocks 8..23 = the raw x pieces, also from the stage-2 GEMM); the tail's epilogue writes the stage-3 conv's operand
        __bf16* ac3 = reinterpret_cast<__bf16*>(ws + p.off_ac3);
        __bf16* at3 = reinterpret_cast<__bf16*>(ws + p.off_at3);
        prof.begin(kRes[3], 3, stream);
        Bf16x3Args ca;
        ca.A = ac3; chain_cfg(h, r, ca, 1, h->res3c_s); ca.bias = h->res[3][0].b; ca.M = L; ca.Mpad = p.Mpc; ca.N = 128; ca.K = 768;
        ca.batch = g; ca.stride = 1; ca.cblocks = 16; ca.Lp = p.Lpc;
        ca.epi = XB_EPI_ELU_SPLIT; ca.S = at3; ca.Spad = p.Mpc; ca.Sphases = 1; ca.Sfront = 0; ca.Sblocks = 24; ca.Sblock0 = 0;
        if (int rc = launch_gemm_bf16x3(ca, stream)) return rc;
        Bf16x3Args ta;
        ta.A = at3; chain_cfg(h, r, ta, 2, h->res3t_s); ta.bias = h->res[3][1].b; ta.M = L; ta.Mpad = p.Mpc; ta.N = 256; ta.K = 384;
        ta.batch = g; ta.stride = 1; ta.cblocks = 24; ta.Lp = p.Mpc;
        ta.epi = XB_EPI_ELU_SPLIT; ta.S = s3; ta.Spad = p.Lp3; ta.Sphases = 8; ta.Sfront = 1;
        if (int rc = launch_gemm_bf16x3(ta, stream)) return rc;
        if (int rc = launch_reflect_front(s3, g, 16, 8, p.Lp3, 8, stream, r.cnp)) return rc;
        prof.end(stream);
    } else if (int rc = enc_gemm_block(h, p, ws, 3, g, stream)) {
        return rc;
    }
    // the strided conv as a split GEMM; behind the fp32 block (no chain3) a stand-alone pass splits its input first: two launches
    prof.begin(kDown[3], r.down3_gemm && !r.chain3 ? 2 : 1, stream);
    if (r.down3_gemm) {
        if (!r.chain3)
            if (int rc = launch_split_phase_major(ws + p.off_r[3], g, L, 256, 8, p.Lp3, s3, stream)) return rc;
        Bf16x3Args ga;
        ga.A = s3; ga.bias = h->down[3].b;
        if (r.chain3) chain_cfg(h, r, ga, 3, h->down3_s); else ga.W = h->down3_s;   // the stand-alone split pass writes bf16 pieces
        ga.M = Lo; ga.Mpad = p.Mp3; ga.N = 512; ga.K = 4096;
        ga.batch = g; ga.stride = 8; ga.cblocks = 16; ga.Lp = p.Lp3;
        ga.epi = XB_EPI_LINEAR; ga.C = out; ga.ldc = 512;
        if (int rc = launch_gemm_bf16x3(ga, stream)) return rc;
    } else if (int rc = enc_gemm_down(h, p, ws, 3, out, g, stream)) {
        return rc;
    }
    prof.end(stream);
    return 0;
}

// The k = 7 conv 512 -> 128 over yw [B][Ty][512] = ELU(lstm + skip) into embw [B][Ty][128]. yp: room for the windowed operand pieces (Lpf rows per clip).
int enc_final_conv(at_encodec* h, const EncRoute& r, const EncPlan& p, float* ws, const float* yw, float* embw, __bf16* yp, int Ty, int Mpf, int Lpf, int B,
                   hipStream_t stream) {
    h->prof.begin("final_conv", r.fin == EncRoute::FIN_SHORT ? 2 : 1, stream);
    if (r.fin == EncRoute::FIN_SHORT) {
        // the reference's short-input rule (pad1d_reflect): zero-extend the rows to pad + 1 = 7, reflect on that copy, keep the first Ty outputs.
        // The copy [B][7][512] lives in the gate buffer, which the LSTM has finished with (B * T * 2048 floats, T >= 2).
        float* yz = ws + p.off_xg;
        AT_CHECK_HIP(hipMemsetAsync(yz, 0, (size_t)B * (kFinPad + 1) * kH * sizeof(float), stream));
        if (int rc = launch_copy_rows(yw, (long long)Ty * kH, yz, (long long)(kFinPad + 1) * kH, Ty, kH, B, stream)) return rc;
        if (int rc = conv_gemm(h->fin, yz, (long long)(kFinPad + 1) * kH, kFinPad + 1, embw, (long long)Ty * kDim, Ty, B, PRO_NONE, nullptr, 0, stream)) return rc;
    } else if (r.fin == EncRoute::FIN_F16X2) {
        // y -> two fp16 pieces in windowed layout (6 reflected front rows), then the k = 7 conv as a windowed split GEMM
        int* range_status = range_site(h, AS_FINAL);
        if (int rc = launch_split_windowed(yw, B, Ty, kH, 1, 6, Lpf, yp, stream, XB_SCHEME_F16X2, XB_F16_ACT_SCALE, range_status)) return rc;
        Bf16x3Args fa;
        fa.A = yp; use_f16x2(fa, h->fin_f, range_status); fa.bias = h->fin.b;
        fa.M = Ty; fa.Mpad = Mpf; fa.N = kDim; fa.K = 7 * kH;
        fa.batch = B; fa.stride = 1; fa.cblocks = kH / 16; fa.Lp = Lpf;
        fa.epi = XB_EPI_LINEAR; fa.C = embw; fa.ldc = kDim;
        if (int rc = launch_gemm_bf16x3(fa, stream)) return rc;
    } else if (int rc = conv_gemm(h->fin, yw, (long long)Ty * kH, Ty, embw, (long long)Ty * kDim, Ty, B, PRO_NONE, nullptr, 0, stream)) {
        return rc;
    }
    h->prof.end(stream);
    return 0;
}

int enc_rvq(at_encodec* h, const float* emb, int B, int Tl, int n_q, int16_t* codes, hipStream_t stream) {
    h->prof.begin("rvq", 1, stream);
    const bool rf = h->opt.rvq_f16x2 && h->cb_f.p;
    int rc = (h->opt.rvq_x3 && h->bf16x3 && h->cb_s)
                 ? launch_rvq_encode_x3(emb, (long long)B * Tl, Tl, h->codebooks, rf ? h->cb_f.p : h->cb_s, (long long)h->n_codebooks * kCodes * kDim, h->e2, n_q,
                                        codes, stream, rf ? XB_SCHEME_F16X2 : XB_SCHEME_BF16X3, XB_F16_ACT_SCALE, h->cb_f.s, range_site(h, AS_RVQ))
                 : launch_rvq_encode(emb, (long long)B * Tl, Tl, h->codebooks, h->e2, n_q, codes, stream);
    h->prof.end(stream);
    return rc;
}

}  // namespace

// One-shot encode (sc == nullptr) and one push of a stream (sc: N new samples behind the state sc->state_in; see StreamState / StreamPlan).
// A push is the one-shot sequence on the window [context | new], with three differences once the stream has started: the window's first two
// frames are dropped in front of the LSTM, the LSTM starts from the carried (h, c), and the final conv runs over [6 carried rows | new rows] and
// keeps the new rows' outputs. The state is read from state_in and written to state_out only.
int encodec_encode_impl(at_encodec_t* h, const float* wav, int B, int N, int n_q, int16_t* codes, int* T_out, float* emb_out, void* workspace,
                        size_t workspace_bytes, at_stream_t stream_, unsigned* status_out, const StreamCall* sc) {
    AT_REQUIRE(h && h->finalized, "model not finalized");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_REQUIRE(wav && codes && workspace, "null pointer");
    const bool mid = sc && sc->started;   // a push behind carried context
    const int n_new = N;
    if (mid) N += kStreamCtx;
    AT_REQUIRE(B >= 1 && N >= 10, "need B >= 1 and N >= 10 samples");
    AT_REQUIRE(n_q >= 1 && n_q <= h->n_codebooks, "n_q out of range for the loaded codebooks");
    hipStream_t stream = (hipStream_t)stream_;
    const StreamPlan sp = sc ? make_stream_plan(B, n_new, sc->started, h->sub_batch) : StreamPlan();
    const EncPlan p = sc ? sp.p : make_plan(B, N, h->sub_batch);
    AT_REQUIRE(workspace_bytes >= (sc ? sp.total_floats : p.total_floats) * sizeof(float), "workspace too small");
    AT_REQUIRE(p.L[3] > 8, "clip too short for the strided convs");
    float* ws = (float*)workspace;
    const int T = p.L[4];                            // frames of the window
    const int Tl = mid ? T - kStreamDrop : T;        // frames that reach the LSTM and leave the call
    const int Ty = mid ? sp.Ty : Tl;                 // rows of the final conv's input
    if (T_out) *T_out = Tl;
    const StreamState sin(sc ? const_cast<void*>(sc->state_in) : nullptr, B), sout(sc ? sc->state_out : nullptr, B);
    const EncHave have{h->down2_s != nullptr, h->down3_s != nullptr, h->res3c_s != nullptr, h->chain_f[0].p != nullptr, h->fin_f.p != nullptr};
    const EncRoute route = enc_route(h->opt, h->bf16x3, have, p, Ty);
    Profiler& prof = h->prof;

    float* x4 = ws + p.off_x4;
    AT_CHECK_HIP(hipMemsetAsync(ws + p.off_sync, 0, 1024 * sizeof(unsigned), stream));   // LSTM flags + the LSTM status word
    AT_CHECK_HIP(hipMemsetAsync(h->range_tab, 0, 64 * sizeof(int), stream));
    if (sc && (mid || !sc->final)) {
        // the window [carried context | new samples] for the conv stack, and the next context: the last 640 samples of it
        prof.begin("stream_state", 1, stream);
        float* win = mid ? ws + sp.off_win : nullptr;
        if (int rc = launch_stream_window(mid ? sin.ctx : nullptr, mid ? kStreamCtx : 0, wav, n_new, win, sc->final ? nullptr : sout.ctx, kStreamCtx, B, stream)) return rc;
        prof.end(stream);
        if (mid) wav = win;
    }
    for (int b0 = 0; b0 < B; b0 += p.G) {
        const int g = (B - b0) < p.G ? (B - b0) : p.G;
        if (int rc = enc_stage0(h, route, p, ws, wav + (long long)b0 * N, g, stream)) return rc;
        if (int rc = enc_stage1(h, route, p, ws, g, stream)) return rc;
        if (int rc = enc_stage2(h, route, p, ws, g, stream)) return rc;
        if (int rc = enc_stage3(h, route, p, ws, x4 + (long long)b0 * T * kH, g, stream)) return rc;
    }
    float* y = ws + p.off_y;
    unsigned* sync = reinterpret_cast<unsigned*>(ws + p.off_sync);   // zeroed at the start of the call (the conv stack's range status lives in it)
    LstmBufs lb{x4, ws + p.off_xg, ws + p.off_xg2, ws + p.off_h0, ws + p.off_h1, ws + p.off_c, y, reinterpret_cast<__bf16*>(ws + p.off_xs), sync};
    LstmCarry carry;
    if (sc) {
        for (int l = 0; l < 2; ++l) { carry.h_init[l] = sin.h[l]; carry.c_init[l] = sin.c[l]; carry.c_final[l] = sout.c[l]; }
        if (mid) {   // drop the window's first two frames: reflect padding has touched them
            prof.begin("stream_state", 1, stream);
            if (int rc = launch_copy_rows(x4 + kStreamDrop * kH, (long long)T * kH, ws + sp.off_x4n, (long long)Tl * kH, Tl, kH, B, stream)) return rc;
            prof.end(stream);
            lb.x = ws + sp.off_x4n;
        }
    }
    if (int rc = lstm_skip(h, h->lstm, lb, B, Tl, sc ? &carry : nullptr, lstm_route(h->opt, h->bf16x3, B, lstm_pipe_eligible(B, Tl), sc != nullptr), range_site(h, AS_LSTM_IH), stream)) return rc;
    float* emb = emb_out ? emb_out : mid ? ws + sp.off_emb : ws + p.off_emb;
    // the final conv's input rows yw [B][Ty][512] and its output embw [B][Ty][128]: mid-stream the 6 carried rows stand in front of the new
    // ones (whatever the kernels reflect in front of THEM only reaches the first 6 outputs, which are not kept)
    const float* yw = y;
    float* embw = emb;
    int Mpf = p.Mpf, Lpf = p.Lpf;
    __bf16* yp = reinterpret_cast<__bf16*>(ws + p.off_xs);
    if (mid) {
        Mpf = sp.Mpf; Lpf = sp.Lpf;
        float* ywm = ws + sp.off_yw;
        prof.begin("stream_state", 2, stream);
        if (int rc = launch_copy_rows(sin.yhist, (long long)kStreamHist * kH, ywm, (long long)Ty * kH, kStreamHist, kH, B, stream)) return rc;
        if (int rc = launch_copy_rows(y, (long long)Tl * kH, ywm + kStreamHist * kH, (long long)Ty * kH, Tl, kH, B, stream)) return rc;
        prof.end(stream);
        yw = ywm; embw = ws + sp.off_embw; yp = reinterpret_cast<__bf16*>(ws + sp.off_yp);
    }
    if (int rc = enc_final_conv(h, route, p, ws, yw, embw, yp, Ty, Mpf, Lpf, B, stream)) return rc;
    if (sc) {
        prof.begin("stream_state", (mid ? 1 : 0) + (sc->final ? 0 : 3), stream);
        if (mid)   // keep the new rows' outputs
            if (int rc = launch_copy_rows(embw + kStreamHist * kDim, (long long)Ty * kDim, emb, (long long)Tl * kDim, Tl, kDim, B, stream)) return rc;
        if (!sc->final) {   // the next push's state: the last 6 conv input rows and the last h of both layers (c: written by the LSTM, context: above)
            if (int rc = launch_copy_rows(yw + (long long)(Ty - kStreamHist) * kH, (long long)Ty * kH, sout.yhist, (long long)kStreamHist * kH, kStreamHist, kH, B, stream)) return rc;
            if (int rc = launch_copy_rows(ws + p.off_h0 + (long long)(Tl - 1) * kH, (long long)Tl * kH, sout.h[0], kH, 1, kH, B, stream)) return rc;
            if (int rc = launch_copy_rows(ws + p.off_h1 + (long long)(Tl - 1) * kH, (long long)Tl * kH, sout.h[1], kH, 1, kH, B, stream)) return rc;
        }
        prof.end(stream);
    }
    if (int rc = enc_rvq(h, emb, B, Tl, n_q, codes, stream)) return rc;
    if (status_out) return launch_status_combine(sync, h->range_tab, status_out, stream);   // LSTM hand-off + every range verdict of the call, RVQ included
    return 0;
}

}  // namespace at
