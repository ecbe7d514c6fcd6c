// Acoustic tokenizer, decode side: codes -> RVQ sum -> first conv -> LSTM -> four upsampling stages (per sub-batch) -> waveform, one-shot or as one
// push of a stream. The kernels of a call are chosen once, by dec_route / lstm_route. Replaces reference AcousticDecoder (audiotoken/decoder.py:50-76).
#include "encodec_handle.h"

namespace at {
namespace {

const char* const kUp[4] = {"dec_up0", "dec_up1", "dec_up2", "dec_up3"};
const char* const kDRes[4] = {"dec_res0", "dec_res1", "dec_res2", "dec_res3"};

// where a sub-batch's samples go: a mid-stream push stores all but the first `skip` of the Lout samples per clip the stack computes
struct DecOut { float* wav; int Lout, skip; long long ostride; bool skip_variant; };

// codes -> z -> x0 = conv0(z) [B][T][512]; a push gathers z behind the carried history and leaves the next history in the state
int dec_front(at_encodec* h, const DecPlan& p, const DecStreamPlan& sp, const DecStreamCall* sc, const DecStreamState& sin, const DecStreamState& sout,
              float* ws, const int64_t* codes, int B, int K, int T, hipStream_t stream) {
    const bool mid = sc && sc->started;
    float* x0 = ws + p.off_x0;
    h->prof.begin("dec_rvq_conv0", 2, stream);
    if (sc) {
        float* zw = ws + sp.off_zw;
        StreamDecStateArgs ga;
        ga.hist_in = mid ? sin.zhist : nullptr; ga.hist = mid ? kDecHist : 0;
        ga.codes = codes; ga.K = K; ga.codebooks = h->codebooks; ga.Tn = T; ga.C = kDim; ga.B = B;
        ga.win = zw; ga.hist_out = sout.zhist; ga.keep = kDecHist;
        if (int rc = launch_stream_dec_state(ga, stream)) return rc;
        if (mid) {   // the carried rows are the left context: output row m reads window rows m .. m + 6, no padding
            GemmArgs a;
            a.X = zw; a.x_bstride = (long long)sp.Tz * kDim; a.Tin = sp.Tz; a.Cin = kDim; a.ldx = kDim;
            a.ktaps = h->dconv0.k; a.stride = 1; a.pad_left = 0; a.pad_mode = 1;
            a.W = h->dconv0.w; a.bias = h->dconv0.b;
            a.C = x0; a.c_bstride = (long long)T * kH; a.ldc = kH;
            a.M = T; a.N = kH; a.K = h->dconv0.k * kDim; a.batch = B; a.pro = PRO_NONE; a.epi = EPI_NONE; a.alpha = 1.0f;
            if (int rc = launch_gemm(a, stream)) return rc;
        } else if (int rc = conv_gemm(h->dconv0, zw, (long long)T * kDim, T, x0, (long long)T * kH, T, B, PRO_NONE, nullptr, 0, stream)) {
            return rc;
        }
    } else {
        float* z = ws + p.off_z;
        if (int rc = launch_rvq_decode(codes, B, K, T, h->codebooks, z, stream)) return rc;
        if (int rc = conv_gemm(h->dconv0, z, (long long)T * kDim, T, x0, (long long)T * kH, T, B, PRO_NONE, nullptr, 0, stream)) return rc;
    }
    h->prof.end(stream);
    return 0;
}

// Stage-0 block (256 channels) as the encoder's stage-3 block: one pass u -> ELU(u) pieces (+ reflect rows) and raw u pieces, the k3 conv and the tail as
// split GEMMs; the tail's ELU -> pieces epilogue writes the NEXT transposed conv's operand (one zero front row): no fp32 block output, no split pass
int dec_chain0(at_encodec* h, const DecPlan& p, float* ws, const float* u, int g, hipStream_t stream) {
    const int Lo = p.L[1];
    __bf16* ac3 = reinterpret_cast<__bf16*>(ws + p.off_dac3);
    __bf16* at3 = reinterpret_cast<__bf16*>(ws + p.off_dat3);
    __bf16* apn = reinterpret_cast<__bf16*>(ws + p.off_ap);
    int* rs = range_site(h, AS_DEC_RES);
    if (int rc = launch_zero_piece_rows(at3, (long long)2 * g * 24, p.dMpc, Lo, p.dMpc, stream)) return rc;
    if (int rc = launch_dec_res256_split(u, g, Lo, ac3, p.dLpc, at3, p.dMpc, XB_F16_ACT_SCALE, rs, stream)) return rc;
    Bf16x3Args ca;
    ca.A = ac3; use_f16x2(ca, h->dchain_f[0], rs); ca.bias = h->dres[0][0].b; ca.M = Lo; ca.Mpad = p.dMpc; ca.N = 128; ca.K = 768;
    ca.batch = g; ca.stride = 1; ca.cblocks = 16; ca.Lp = p.dLpc;
    ca.epi = XB_EPI_ELU_SPLIT; ca.S = at3; ca.Spad = p.dMpc; ca.Sphases = 1; ca.Sfront = 0; ca.Sblocks = 24; ca.Sblock0 = 0;
    if (int rc = launch_gemm_bf16x3(ca, stream)) return rc;
    // the next stage's operand: [2][g][16][Lpu][16], row t at index t + 1; row 0 and the rows past the data zero
    if (int rc = launch_zero_piece_rows(apn, (long long)2 * g * 16, p.Lpu[1], 0, 1, stream)) return rc;
    if (int rc = launch_zero_piece_rows(apn, (long long)2 * g * 16, p.Lpu[1], Lo + 1, p.Lpu[1], stream)) return rc;
    Bf16x3Args ta;
    ta.A = at3; use_f16x2(ta, h->dchain_f[1], rs); ta.bias = h->dres[0][1].b; ta.M = Lo; ta.Mpad = p.dMpc; ta.N = 256; ta.K = 384;
    ta.batch = g; ta.stride = 1; ta.cblocks = 24; ta.Lp = p.dMpc;
    ta.epi = XB_EPI_ELU_SPLIT; ta.S = apn; ta.Spad = p.Lpu[1]; ta.Sphases = 1; ta.Sfront = 1;
    return launch_gemm_bf16x3(ta, stream);
}

// Stage s: transposed conv of the (already ELU'd) rows `in` [g][L[s]][512 >> s], then the block; returns the block's output r[s] (after the stage-0
// chain nothing lies there: its output is stage 1's operand pieces in `ap`, which stage 1 then reads instead of `in`)
int dec_stage(at_encodec* h, const DecRoute& r, const DecPlan& p, float* ws, int s, const float* in, int g, hipStream_t stream) {
    Profiler& prof = h->prof;
    const int Cin = kH >> s, Co = Cin / 2, Li = p.L[s], Lo = p.L[s + 1];
    float *u = ws + p.off_u[s], *rb = ws + p.off_r[s];
    prof.begin(kUp[s], 2, stream);
    // ConvTranspose1d(k = 2r, stride r) of the (already ELU'd) input, trimmed right by r, as one GEMM with N = r*Cout:
    // out[t][p*Cout + co] = x[t-1].W[:, co, p+r] + x[t].W[:, co, p]; [Li][r*Cout] is [Lo][Cout] in memory.
    if (r.up_gemm[s]) {
        // as a two-tap windowed split GEMM on the fp16 scheme: the (already ELU'd) input -> pieces with ONE ZERO front row (x[-1] = 0)
        __bf16* ap = reinterpret_cast<__bf16*>(ws + p.off_ap);
        int* range_status = range_site(h, AS_DEC_UP);
        if (!(s == 1 && r.chain0))   // (after the stage-0 chain the block's tail GEMM has already written these pieces)
            if (int rc = launch_split_windowed(in, g, Li, Cin, 1, 1, p.Lpu[s], ap, stream, XB_SCHEME_F16X2, XB_F16_ACT_SCALE, range_status, 0)) return rc;
        Bf16x3Args ua;
        ua.A = ap; use_f16x2(ua, h->dup_f[s], range_status); ua.bias = h->dup[s].b;
        ua.M = Li; ua.Mpad = p.Mpu[s]; ua.N = kRatiosDec[s] * Co; ua.K = 2 * Cin;
        ua.batch = g; ua.stride = 1; ua.cblocks = Cin / 16; ua.Lp = p.Lpu[s];
        ua.epi = XB_EPI_LINEAR; ua.C = u; ua.ldc = ua.N;
        if (int rc = launch_gemm_bf16x3(ua, stream)) return rc;
    } else if (int rc = conv_gemm(h->dup[s], in, (long long)Li * Cin, Li, u, (long long)Lo * Co, Li, g, PRO_NONE, nullptr, 0, stream, 0)) {
        return rc;
    }
    prof.end(stream);
    prof.begin(kDRes[s], 1, stream);
    if (s == 0 && r.chain0) {
        if (int rc = dec_chain0(h, p, ws, u, g, stream)) return rc;
    } else if (r.res[s] != RES_GEMM) {
        Res64Args ra;
        ra.x = u; ra.out = rb; ra.w3 = h->dres[s][0].w; ra.b3 = h->dres[s][0].b; ra.wt = h->dres[s][1].w; ra.bt = h->dres[s][1].b;
        ra.B = g; ra.L = Lo;
        if (r.res_f16[s]) {   // the blocks' own contractions on the two-piece fp16 scheme, as in the encoder
            ra.scheme = XB_SCHEME_F16X2; ra.act_scale = XB_F16_ACT_SCALE; ra.w3_scale = h->dres_fs[s][0]; ra.wt_scale = h->dres_fs[s][1];
            ra.status = range_site(h, AS_DEC_RES);
        }
        if (int rc = launch_res_kernel(r.res[s], ra, stream)) return rc;
    } else {
        // the last block's output goes to conv_last, which applies the ELU itself
        if (int rc = resblock(h->dres[s], u, ws + p.off_h[s], rb, Lo, g, stream, s < 3 ? EPI_ELU : EPI_NONE)) return rc;
    }
    prof.end(stream);
    return 0;
}

// rows `in` [g][L[3]][64] (fused: stage 3 and the final conv in one kernel) or the last block's output [g][L[4]][32] -> samples
int dec_tail(at_encodec* h, const DecRoute& r, const DecPlan& p, const float* in, const DecOut& o, int g, hipStream_t stream) {
    h->prof.begin("dec_tail", 1, stream);
    if (r.tail == DecRoute::TAIL_CONV_LAST) {
        if (int rc = o.skip_variant ? launch_conv_last_skip(in, h->dlast.w, h->dlast.b, o.wav, g, o.Lout, o.skip, o.ostride, stream)
                                    : launch_conv_last(in, h->dlast.w, h->dlast.b, o.wav, g, o.Lout, stream)) return rc;
    } else {
        DecTailArgs da;
        da.x = in; da.out = o.wav;
        da.wu = h->dup[3].w; da.bu = h->dup[3].b; da.w3 = h->dres[3][0].w; da.b3 = h->dres[3][0].b;
        da.wt = h->dres[3][1].w; da.bt = h->dres[3][1].b; da.wl = h->dlast.w; da.bl = h->dlast.b;
        da.B = g; da.L = p.L[3];
        if (r.tail == DecRoute::TAIL_FUSED_X2) {
            da.act_scale = XB_F16_ACT_SCALE; da.wu_scale = h->dtail_up_fs; da.w3_scale = h->dres_fs[3][0]; da.wt_scale = h->dres_fs[3][1];
            da.status = range_site(h, AS_DEC_RES);
            if (int rc = o.skip_variant ? launch_seanet_dectail_x2_skip(da, o.skip, o.ostride, stream) : launch_seanet_dectail_x2(da, stream)) return rc;
        } else if (int rc = o.skip_variant ? launch_seanet_dectail_skip(da, o.skip, o.ostride, stream) : launch_seanet_dectail(da, stream)) {
            return rc;
        }
    }
    h->prof.end(stream);
    return 0;
}

}  // namespace

// One-shot decode (sc == nullptr) or one push of a stream: T new frames. A push differs in three places: the state kernel gathers z behind the carried
// history (and the first conv then needs no padding), the LSTM starts from the carried (h, c), and the upsampling stack runs on Tw = T + 2 rows with
// the tail kernels' skip / stride variant dropping the first 640 samples. Everything else is the one-shot code on the window.
int encodec_decode_impl(at_encodec_t* h, const int64_t* codes, int B, int K, int T, float* wav, void* workspace, size_t workspace_bytes,
                        at_stream_t stream_, uint32_t* status_dev, const DecStreamCall* sc) {
    AT_REQUIRE(h && h->finalized && h->has_decoder, "model not finalized with a decoder");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_REQUIRE(codes && wav && workspace, "null pointer");
    const bool mid = sc && sc->started;
    AT_REQUIRE(B >= 1 && T >= (mid ? 1 : kDecFirstFrames) && K >= 1 && K <= h->n_codebooks, "bad B/T/K");
    hipStream_t stream = (hipStream_t)stream_;
    const DecStreamPlan sp = sc ? make_dec_stream_plan(B, T, mid, h->sub_batch) : DecStreamPlan();
    const DecPlan p = sc ? sp.p : make_dec_plan(B, T, h->sub_batch);
    AT_REQUIRE(workspace_bytes >= (sc ? sp.total_floats : p.total_floats) * sizeof(float), "workspace too small");
    float* ws = (float*)workspace;
    const int Tw = sc ? sp.Tw : T;   // rows through the upsampling stack
    const DecStreamState sin(sc ? const_cast<void*>(sc->state_in) : nullptr, B), sout(sc ? sc->state_out : nullptr, B);
    DecHave have;
    have.dtail_up_fs = h->dtail_up_fs > 0.f;
    for (int s = 0; s < 4; ++s) {
        have.dres_fs[s] = h->dres_fs[s][0] > 0.f;
        if (s < 3) have.dup_f[s] = h->dup_f[s].p != nullptr;
        if (s < 2) have.dchain_f[s] = h->dchain_f[s].p != nullptr;
    }
    const DecRoute route = dec_route(h->opt, h->bf16x3, have, p);
    Profiler& prof = h->prof;   // same HIP-event taps as the encoder (at_encodec_profile / at_encodec_profile_read)
    if (int rc = dec_front(h, p, sp, sc, sin, sout, ws, codes, B, K, T, stream)) return rc;
    float* y = ws + p.off_y;
    unsigned* sync = reinterpret_cast<unsigned*>(ws + p.off_sync);
    AT_CHECK_HIP(hipMemsetAsync(sync, 0, 1024 * sizeof(unsigned), stream));
    AT_CHECK_HIP(hipMemsetAsync(h->range_tab, 0, 64 * sizeof(int), stream));
    LstmCarry carry;
    if (sc)
        for (int l = 0; l < 2; ++l) { carry.h_init[l] = sin.h[l]; carry.c_init[l] = sin.c[l]; carry.c_final[l] = sout.c[l]; }
    // every activation that is only consumed through ELU is stored already ELU'd (once per element, in the producer's
    // epilogue) so the transposed convs run the plain-linear GEMM path: y (LSTM + skip) and the block outputs of stages 0-2
    const LstmBufs lb{ws + p.off_x0, ws + p.off_xg, ws + p.off_xg2, ws + p.off_h0, ws + p.off_h1, ws + p.off_c, y, reinterpret_cast<__bf16*>(ws + p.off_xs), sync};
    if (int rc = lstm_skip(h, h->dlstm, lb, B, T, sc ? &carry : nullptr, lstm_route(h->opt, h->bf16x3, B, lstm_pipe_eligible(B, T), sc != nullptr), range_site(h, AS_DEC_LSTM_IH), stream)) return rc;
    if (sc) {   // [carried rows | new rows] of ELU(lstm + skip), the next push's two rows and the last h of both layers (c: written by the LSTM)
        StreamDecStateArgs ya;
        ya.hist_in = mid ? sin.yctx : nullptr; ya.hist = mid ? kDecCtx : 0;
        ya.src = y; ya.Tn = T; ya.C = kH; ya.B = B;
        ya.win = mid ? ws + sp.off_yw : nullptr; ya.hist_out = sout.yctx; ya.keep = kDecCtx;
        ya.h_src[0] = ws + p.off_h0; ya.h_src[1] = ws + p.off_h1; ya.h_out[0] = sout.h[0]; ya.h_out[1] = sout.h[1];
        prof.begin("stream_state", 1, stream);
        if (int rc = launch_stream_dec_state(ya, stream)) return rc;
        prof.end(stream);
        if (mid) y = ws + sp.off_yw;
    }
    DecOut out;
    out.Lout = p.L[4];
    out.skip = mid ? kDecCtx * kHop : 0;
    out.ostride = (long long)out.Lout - out.skip;
    out.skip_variant = mid || h->opt.dec_skip_twin;
    const int stages = route.tail == DecRoute::TAIL_CONV_LAST ? 4 : 3;
    for (int b0 = 0; b0 < B; b0 += p.G) {
        const int g = (B - b0) < p.G ? (B - b0) : p.G;
        const float* in = y + (long long)b0 * Tw * kH;
        for (int s = 0; s < stages; ++s) {
            if (int rc = dec_stage(h, route, p, ws, s, in, g, stream)) return rc;
            in = ws + p.off_r[s];
        }
        out.wav = wav + (long long)b0 * out.ostride;
        if (int rc = dec_tail(h, route, p, in, out, g, stream)) return rc;
    }
    if (status_dev) return launch_status_combine(sync, h->range_tab, status_dev, stream);   // LSTM hand-off + every range verdict of the call
    return 0;
}

}  // namespace at
