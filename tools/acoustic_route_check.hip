// The acoustic route functions (audiotoken_amd/csrc/encodec_plan.h, pure host code: enc_route, dec_route, lstm_route) against the five length predicates that
// tests/acoustic_routes.py documents, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer. Built and run by
// `make -C audiotoken_amd/csrc route_asan`; tests/test_acoustic_route_host_cpu.py runs it over every length of acoustic_routes.LENGTHS.
//   acoustic_route_check N [N ...]   prints "N a b c d e" per length (default options, every split weight present), status 1 on a mismatch
#include <cstdio>
#include <cstdlib>

#include "../audiotoken_amd/csrc/encodec_plan.h"

using namespace at;

static int check(int N, int B) {
    const EncPlan p = make_plan(B, N, kSubBatchDefault);
    const int* L = p.L;
    const EncRoute r = enc_route(Options(), true, EncHave{true, true, true, true, true}, p, L[4]);
    const bool want[5] = {N % 2 == 0, L[1] % 4 == 0 && L[1] >= 8, L[2] % 5 == 0 && L[2] >= 10, L[3] % 8 == 0 && L[3] >= 16, L[4] > 6};
    const bool got[5] = {r.fused0, r.stage1_fused, r.down2_gemm, r.down3_gemm, r.fin == EncRoute::FIN_F16X2};
    int bad = 0;
    for (int k = 0; k < 5; ++k) bad += got[k] != want[k];
    bad += r.chain3 != (want[2] && want[3]);
    bad += r.cf != true || r.cnp != 2 || r.res1 != RES64_X3 || r.res2 != RES128_RS || r.down64 != (L[1] % 4 == 0);
    bad += (r.fin == EncRoute::FIN_SHORT) != (L[4] <= 6);
    // without bf16x3 nothing runs on split operands, whatever the options say; a short clip keeps the short-input rule
    const EncRoute f = enc_route(Options(), false, EncHave{}, p, L[4]);
    bad += f.stage1_fused || f.down2_gemm || f.chain3 || f.down3_gemm || f.cf || f.cnp != 3 || f.fin == EncRoute::FIN_F16X2 || f.fused0 != want[0];
    if (B == 1) std::printf("%d %d %d %d %d %d\n", N, (int)got[0], (int)got[1], (int)got[2], (int)got[3], (int)got[4]);
    if (bad) std::printf("MISMATCH at N = %d, B = %d\n", N, B);
    return bad;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int i = 1; i < argc; ++i)
        for (int B : {1, 3, 81, 300}) bad += check(std::atoi(argv[i]), B);   // the route does not depend on the batch
    {   // the decoder: defaults take the chain and the fused fp16 tail; a stream's one-row push cannot run stage 0's transposed conv as a windowed GEMM
        DecHave all;
        all.dtail_up_fs = all.dchain_f[0] = all.dchain_f[1] = true;
        for (int s = 0; s < 4; ++s) { all.dres_fs[s] = true; if (s < 3) all.dup_f[s] = true; }
        const DecRoute d7 = dec_route(Options(), true, all, make_dec_plan(2, 7, kSubBatchDefault));
        bad += !d7.chain0 || d7.tail != DecRoute::TAIL_FUSED_X2 || !d7.up_gemm[0] || !d7.up_gemm[1] || !d7.up_gemm[2] || d7.up_gemm[3];
        bad += d7.res[1] != RES128_RS || d7.res[2] != RES64_X3 || d7.res[0] != RES_GEMM || d7.res[3] != RES_GEMM;
        const DecRoute d1 = dec_route(Options(), true, all, make_dec_plan(2, 1, kSubBatchDefault));
        bad += d1.up_gemm[0] || !d1.up_gemm[1] || !d1.chain0;
        Options o;
        o.fused_dectail = false;
        bad += dec_route(o, true, all, make_dec_plan(2, 7, kSubBatchDefault)).tail != DecRoute::TAIL_CONV_LAST;
        bad += dec_route(Options(), false, DecHave{}, make_dec_plan(2, 7, kSubBatchDefault)).tail != DecRoute::TAIL_FUSED;
        if (bad) std::printf("decoder route mismatch\n");
    }
    {   // the LSTM: defaults pipeline small batches; a carried state without the fp16-scheme recurrence runs the fp32 persistent kernel
        Options o;
        o.persistent_lstm = true;   // what finalize() sets on a 256-CU device
        int lb = 0;
        lb += lstm_route(o, true, 3, true, false).rec != LstmRoute::REC_PIPE || lstm_route(o, true, 3, true, true).rec != LstmRoute::REC_PIPE;
        lb += lstm_route(o, true, 3, false, false).rec != LstmRoute::REC_SEQ_F16X2 || lstm_route(o, true, kPipeMaxClips + 1, true, false).rec != LstmRoute::REC_SEQ_F16X2;
        lb += lstm_route(o, true, 3, true, false).ih != LstmRoute::IH_F16X2 || lstm_route(o, false, 3, true, false).ih != LstmRoute::IH_F32;
        lb += lstm_route(o, false, 3, true, false).rec != LstmRoute::REC_SEQ_F32;
        o.lstm_f16x2 = false;
        lb += lstm_route(o, true, 3, true, false).rec != LstmRoute::REC_SEQ_BF16X3;   // one-shot: the three-piece bf16 recurrence
        lb += lstm_route(o, true, 3, true, true).rec != LstmRoute::REC_SEQ_F32;       // carried state: it has no state variant
        o.ih_f16x2 = false;
        lb += lstm_route(o, true, 3, true, true).ih != LstmRoute::IH_BF16X3;
        o.persistent_lstm = false;
        lb += lstm_route(o, true, 3, true, true).rec != LstmRoute::REC_STEPWISE;
        if (lb) std::printf("LSTM route mismatch\n");
        bad += lb;
    }
    if (bad) return 1;
    std::printf("acoustic route checks: ok\n");
    return 0;
}
