// Acoustic tokenizer (EnCodec 24 kHz): the handle, its weight types, and what encodec.hip (C ABI), encodec_finalize.hip, encodec_encode.hip,
// encodec_decode.hip and encodec_lstm.hip share.
//
// Data layout: every activation is time-major / channels-last [clip][t][c] so that conv windows are contiguous
// (see at_common.h). Weights are repacked once at finalize():
//   Conv1d  [Cout][Cin][k]      -> [Cout][k*Cin]            (tap-major rows, matches the window order)
//   ConvTr  [Cin][Cout][k=2s]   -> [s*Cout][2*Cin]          (phase p row block: [W[:, :, p+s] | W[:, :, p]])
//   LSTM    [4H][H] gate blocks -> rows 4*j + g             (gates of one unit adjacent; see lstm_step_kernel)
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/audiotoken_hip.h"
#include "at_common.h"
#include "encodec_kernels.h"
#include "encodec_plan.h"
#include "semantic_handle.h"   // HostTensor, stage_tensor, device_exists

namespace at {

constexpr bool kBf16x3AcousticDefault = true;

struct ConvW {
    const float* w = nullptr;
    const float* b = nullptr;
    int cin = 0, cout = 0, k = 0, stride = 1;
};
// one 2-layer LSTM: fp32 weights in gate-interleaved rows, and with bf16x3 the input projections as operand pieces
struct LstmW {
    const float *wih[2] = {}, *whh[2] = {}, *bih[2] = {}, *bhh[2] = {};
    const __bf16* wih_s[2] = {nullptr, nullptr};     // three bf16 pieces
    const piece_t* wih_f[2] = {nullptr, nullptr};    // two fp16 pieces (gemm_bf16x3.h, XB_SCHEME_F16X2) of W * wih_fs
    float wih_fs[2] = {1.f, 1.f};
    float whh_fs[2] = {0.f, 0.f};   // W_hh scales of the fp16-scheme recurrence (the kernel splits W_hh itself, once per launch)
};

}  // namespace at

struct at_encodec {
    int device = 0;
    bool finalized = false;
    bool has_decoder = false;
    std::map<std::string, at::HostTensor> staged;
    float* blob = nullptr;
    size_t blob_floats = 0;
    at::Options opt;
    bool bf16x3 = false;            // plain linear layers (LSTM input projections) on the split-bf16 GEMM ($AUDIOTOKEN_BF16X3_ACOUSTIC)
    // encoder
    at::ConvW conv0, res[4][3], down[4], fin;
    at::LstmW lstm;
    const float* sc0_w = nullptr;   // stage 0: shortcut folded into conv0, [32][7] weights then [32] bias (Stage0Args::wsc0 / bsc0)
    // fused residual blocks on the fp16 scheme (option "res_f16x2"): power-of-two scales of [conv3, tail] per stage, encoder / decoder
    float res_fs[4][2] = {}, dres_fs[4][2] = {};
    float down_fs[4] = {};    // strided convs (stage-1 fused kernel on the fp16 scheme)
    const __bf16 *down2_s = nullptr, *down3_s = nullptr, *res3c_s = nullptr, *res3t_s = nullptr;   // the stage 2-3 GEMM chain's weights as three bf16 pieces
    at::SplitW chain_f[4];          // ... and as two fp16 pieces: down2, res3 conv3, res3 tail, down3 (option "chain_f16x2")
    at::SplitW fin_f;               // final conv weight [128][7 * 512] as two fp16 pieces, K-blocks in window order (option "fin_f16x2")
    // quantiser
    const float* codebooks = nullptr;  // [n_cb][1024][128]
    const float* e2 = nullptr;         // [n_cb][1024]
    int n_codebooks = 0;
    const __bf16* cb_s = nullptr;   // codebooks as 3 bf16 pieces [3][n_cb * 1024][128]
    at::SplitW cb_f;                // codebooks * s as 2 fp16 pieces [2][n_cb * 1024][128] (option "rvq_f16x2")
    // decoder
    at::ConvW dconv0, dup[4], dres[4][3], dlast;
    at::LstmW dlstm;
    at::SplitW dup_f[3];            // transposed convs [r * Cout][2 * Cin] as two fp16 pieces, window order (option "up_f16x2")
    at::SplitW dchain_f[2];         // stage-0 block (option "dec_chain"): its k3 conv [128][3 * 256] (window order) and tail [256][128 + 256] as two fp16 pieces (scales = dres_fs[0])
    float dtail_up_fs = 0.f;        // power-of-two scale of the last transposed conv's weights for the fused tail kernel
    at::Profiler prof;
    std::vector<void*> extra_allocs;
    int* range_tab = nullptr;   // device, {flag, census} per AcSite, zeroed at the start of every encode / decode (at_encodec_range_report reads it)
    int sub_batch = at::sub_batch();   // clips per pass through the conv stack: bounds the workspace (option "subbatch")
    unsigned lstm_spin_limit = 1u << 18;   // option "lstm_spin_limit": flag polls before a persistent-LSTM workgroup gives up
    // streaming encode: what the host knows about every state buffer it has reset or written (the state itself is device memory; this is
    // what lets a push be refused without a device synchronisation)
    struct StreamInfo { int B = 0; bool started = false, finished = false, decode = false; };   // decode: a state of at_encodec_decode_stream_*
    std::map<const void*, StreamInfo> streams;
};

namespace at {

// Range table of a handle (device, zeroed per call): one {flag word, census word} pair per SITE = per place where activations are split into
// fp16 pieces. A split writer ORs XB_STATUS_F16_OVERFLOW into its site's flag word and raises the census word to the largest |x * scale| it saw
// (split_scheme.h, range_publish); at_encodec_range_report() returns the census, i.e. the measured headroom to 65504 per site.
enum AcSite { AS_STAGE0 = 0, AS_RES1, AS_DOWN1, AS_RES2, AS_DOWN2, AS_RES3_CONV, AS_RES3_TAIL, AS_LSTM_IH, AS_FINAL, AS_RVQ,
              AS_DEC_LSTM_IH, AS_DEC_UP, AS_DEC_RES, AC_NSITES };
inline int* range_site(const at_encodec* h, int site) { return h->range_tab + 2 * site; }
// status word of the *_checked entry points from the LSTM's sync words and the range table (encodec.hip)
int launch_status_combine(const unsigned* sync, const int* range_tab, unsigned* out, hipStream_t stream);

// a split GEMM on the two-piece fp16 scheme: weight pieces w, activations split with XB_F16_ACT_SCALE, range verdict into `status`
inline void use_f16x2(Bf16x3Args& a, const SplitW& w, int* status) {
    a.W = w.p; a.scheme = XB_SCHEME_F16X2; a.acc_scale = 1.0f / (XB_F16_ACT_SCALE * w.s); a.split_scale = XB_F16_ACT_SCALE; a.status = status;
}

// encodec_lstm.hip: building blocks of both sides
int conv_gemm(const ConvW& c, const float* X, long long x_bstride, int Tin, float* C, long long c_bstride, int M, int batch,
              int pro, const float* R, long long r_bstride, hipStream_t stream, int pad_mode = 1, int epi = EPI_NONE);
int resblock(const ConvW (&r)[3], const float* x, float* hbuf, float* out, int L, int batch, hipStream_t stream, int epi = EPI_NONE);
int launch_res_kernel(ResKernel k, const Res64Args& ra, hipStream_t stream);   // a fused 64- / 128-channel block (not RES_GEMM)
// encodec_encode.hip
int encodec_encode_impl(at_encodec_t* h, const float* wav, int B, int N, int n_q, int16_t* codes, int* T_out, float* emb_out, void* workspace,
                        size_t workspace_bytes, at_stream_t stream_, unsigned* status_out, const StreamCall* sc);
// encodec_decode.hip
int encodec_decode_impl(at_encodec_t* h, const int64_t* codes, int B, int K, int T, float* wav, void* workspace, size_t workspace_bytes,
                        at_stream_t stream_, uint32_t* status_dev, const DecStreamCall* sc);

// encodec_lstm.hip. 2-layer LSTM + skip over [B][T][512]: y = ELU(lstm(x) + x). xg / xg2 / c / h0 / h1 / xs are scratch; h0 / h1 keep the layers' outputs.
struct LstmCarry { const float* h_init[2]; const float* c_init[2]; float* c_final[2]; };
struct LstmBufs {
    const float* x;          // [B][T][512]
    float *xg, *xg2;         // input gates [B][T][2048]; xg2: layer 2's, for the pipelined launch (plans hold it for B <= kPipeMaxClips only)
    float *h0, *h1, *c, *y;
    __bf16* xs;              // split copy of a layer's input
    unsigned* sync;          // hand-off flags and the LSTM status word, zeroed by the caller
};
int lstm_skip(at_encodec* h, const LstmW& w, const LstmBufs& b, int B, int T, const LstmCarry* carry, LstmRoute route, int* range_status, hipStream_t stream);

}  // namespace at
