// Acoustic tokenizer: weight intake. at_encodec_finalize repacks the staged tensors into one device blob (layouts: encodec_handle.h) and, with
// bf16x3, makes the 16-bit operand pieces and power-of-two scales of every weight that runs on the matrix cores.
#include <cmath>
#include <cstring>

#include "encodec_handle.h"

using namespace at;

namespace {

const HostTensor* find(const at_encodec* h, const std::string& name) {
    auto it = h->staged.find(name);
    return it == h->staged.end() ? nullptr : &it->second;
}

struct Packer {
    std::vector<float> host;
    size_t add(const std::vector<float>& v) {
        size_t off = host.size();
        host.insert(host.end(), v.begin(), v.end());
        while (host.size() % 4) host.push_back(0.f);  // keep every tensor 16-byte aligned
        return off;
    }
};

// where every packed tensor lies in the host blob (floats)
struct Off { size_t w, b; };
struct Offsets {
    Off conv0, res[4][3], down[4], fin;
    size_t lstm[2][4];
    size_t cb, e2;
    int ncb;
    Off dconv0 = {}, dup[4] = {}, dres[4][3] = {}, dlast = {};
    size_t dlstm[2][4] = {};
};

// Conv1d weight [cout][cin][k] -> [cout][k][cin]
bool pack_conv(const at_encodec* h, const std::string& prefix, int cin, int cout, int k, Packer& p, Off& o) {
    const HostTensor* w = find(h, prefix + ".weight");
    const HostTensor* b = find(h, prefix + ".bias");
    if (!w || !b) { set_error("missing tensor " + prefix + ".{weight,bias}"); return false; }
    if (w->shape != std::vector<int64_t>{cout, cin, k} || b->shape != std::vector<int64_t>{cout}) {
        set_error("bad shape for " + prefix);
        return false;
    }
    std::vector<float> out((size_t)cout * k * cin);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < k; ++t) out[((size_t)co * k + t) * cin + ci] = w->data[((size_t)co * cin + ci) * k + t];
    o.w = p.add(out);
    o.b = p.add(b->data);
    return true;
}

// ConvTranspose1d weight [cin][cout][k = 2s] -> rows (p*cout + co), cols [x[t-1] block | x[t] block]
bool pack_convtr(const at_encodec* h, const std::string& prefix, int cin, int cout, int s, Packer& p, Off& o) {
    const HostTensor* w = find(h, prefix + ".weight");
    const HostTensor* b = find(h, prefix + ".bias");
    if (!w || !b) { set_error("missing tensor " + prefix + ".{weight,bias}"); return false; }
    const int k = 2 * s;
    if (w->shape != std::vector<int64_t>{cin, cout, k} || b->shape != std::vector<int64_t>{cout}) {
        set_error("bad shape for " + prefix);
        return false;
    }
    std::vector<float> out((size_t)s * cout * 2 * cin);
    for (int ph = 0; ph < s; ++ph)
        for (int co = 0; co < cout; ++co) {
            float* row = &out[((size_t)ph * cout + co) * 2 * cin];
            for (int ci = 0; ci < cin; ++ci) {
                row[ci] = w->data[((size_t)ci * cout + co) * k + ph + s];  // x[t-1] contributes tap p+s
                row[cin + ci] = w->data[((size_t)ci * cout + co) * k + ph];  // x[t] contributes tap p
            }
        }
    std::vector<float> bias((size_t)s * cout);
    for (int ph = 0; ph < s; ++ph)
        for (int co = 0; co < cout; ++co) bias[(size_t)ph * cout + co] = b->data[co];
    o.w = p.add(out);
    o.b = p.add(bias);
    return true;
}

// residual block tail: [W1 (C x C/2) | Wsc (C x C)] rows concatenated along K, biases summed
bool pack_res_tail(const at_encodec* h, const std::string& p1, const std::string& psc, int C, Packer& p, Off& o) {
    const HostTensor* w1 = find(h, p1 + ".weight");
    const HostTensor* b1 = find(h, p1 + ".bias");
    const HostTensor* ws = find(h, psc + ".weight");
    const HostTensor* bs = find(h, psc + ".bias");
    if (!w1 || !b1 || !ws || !bs) { set_error("missing tensor " + p1 + " / " + psc); return false; }
    if (w1->shape != std::vector<int64_t>{C, C / 2, 1} || ws->shape != std::vector<int64_t>{C, C, 1} ||
        b1->shape != std::vector<int64_t>{C} || bs->shape != std::vector<int64_t>{C}) {
        set_error("bad shape for " + p1 + " / " + psc);
        return false;
    }
    const int K = C / 2 + C;
    std::vector<float> w((size_t)C * K), b(C);
    for (int co = 0; co < C; ++co) {
        for (int ci = 0; ci < C / 2; ++ci) w[(size_t)co * K + ci] = w1->data[(size_t)co * (C / 2) + ci];
        for (int ci = 0; ci < C; ++ci) w[(size_t)co * K + C / 2 + ci] = ws->data[(size_t)co * C + ci];
        // reference order: shortcut(x) + block(x) -> (Wsc.x + bsc) + (W1.h + b1); the GEMM adds ONE bias to the
        // full dot product, so the two biases are pre-added (a 1-ulp reassociation, inside the 1e-3 budget)
        b[co] = bs->data[co] + b1->data[co];
    }
    o.w = p.add(w);
    o.b = p.add(b);
    return true;
}

// a SEANet residual block of C channels under `base`: conv3 -> res[0]; [W1 | Wsc] -> res[1] (res[2] names the same tensor)
bool pack_block(const at_encodec* h, const std::string& base, int C, Packer& p, Off (&res)[3]) {
    if (!pack_conv(h, base + ".block.1.conv.conv", C, C / 2, 3, p, res[0])) return false;
    if (!pack_res_tail(h, base + ".block.3.conv.conv", base + ".shortcut.conv.conv", C, p, res[1])) return false;
    res[2] = res[1];
    return true;
}

bool pack_lstm(const at_encodec* h, const std::string& prefix, Packer& p, size_t off[2][4]) {
    for (int l = 0; l < 2; ++l) {
        const char* names[4] = {"weight_ih", "weight_hh", "bias_ih", "bias_hh"};
        for (int which = 0; which < 4; ++which) {
            const std::string key = prefix + ".lstm." + names[which] + "_l" + std::to_string(l);
            const HostTensor* t = find(h, key);
            if (!t) { set_error("missing tensor " + key); return false; }
            const bool is_w = which < 2;
            if ((is_w && t->shape != std::vector<int64_t>{4 * kH, kH}) || (!is_w && t->shape != std::vector<int64_t>{4 * kH})) {
                set_error("bad shape for " + key);
                return false;
            }
            const size_t cols = is_w ? kH : 1;
            std::vector<float> out(t->data.size());
            for (int g = 0; g < 4; ++g)
                for (int j = 0; j < kH; ++j)
                    std::memcpy(&out[((size_t)j * 4 + g) * cols], &t->data[((size_t)g * kH + j) * cols], cols * sizeof(float));
            off[l][which] = p.add(out);
        }
    }
    return true;
}

// codebooks: consecutive layers 0..n-1, and |e|^2 per code (supplied as "...e2" or computed here)
int pack_codebooks(at_encodec* h, Packer& p, Offsets& o) {
    int ncb = 0;
    while (find(h, "quantizer.vq.layers." + std::to_string(ncb) + "._codebook.embed")) ++ncb;
    AT_REQUIRE(ncb >= 1, "no codebooks (quantizer.vq.layers.0._codebook.embed) supplied");
    std::vector<float> cbs((size_t)ncb * kCodes * kDim), e2s((size_t)ncb * kCodes);
    for (int q = 0; q < ncb; ++q) {
        const std::string key = "quantizer.vq.layers." + std::to_string(q) + "._codebook.embed";
        const HostTensor* t = find(h, key);
        AT_REQUIRE(t->shape == (std::vector<int64_t>{kCodes, kDim}), "bad codebook shape");
        std::memcpy(&cbs[(size_t)q * kCodes * kDim], t->data.data(), (size_t)kCodes * kDim * sizeof(float));
        const HostTensor* e = find(h, key.substr(0, key.size() - 5) + "e2");
        if (e) {
            AT_REQUIRE(e->shape == (std::vector<int64_t>{kCodes}), "bad e2 shape");
            std::memcpy(&e2s[(size_t)q * kCodes], e->data.data(), kCodes * sizeof(float));
        } else {
            for (int n = 0; n < kCodes; ++n) {
                float acc = 0.f;
                for (int k = 0; k < kDim; ++k) { const float v = t->data[(size_t)n * kDim + k]; acc += v * v; }
                e2s[(size_t)q * kCodes + n] = acc;
            }
        }
    }
    o.cb = p.add(cbs);
    o.e2 = p.add(e2s);
    o.ncb = ncb;
    return 0;
}

// every staged tensor, repacked, into the host blob
int pack_host(at_encodec* h, bool with_decoder, Packer& p, Offsets& o) {
    // conv0 keeps [32][7] (Cin = 1): tap-major == torch layout
    if (!pack_conv(h, "encoder.model.0.conv.conv", 1, 32, 7, p, o.conv0)) return -1;
    int C = 32, idx = 1;
    for (int s = 0; s < 4; ++s) {
        if (!pack_block(h, "encoder.model." + std::to_string(idx), C, p, o.res[s])) return -1;
        if (!pack_conv(h, "encoder.model." + std::to_string(idx + 2) + ".conv.conv", C, 2 * C, 2 * kRatiosEnc[s], p, o.down[s])) return -1;
        C *= 2;
        idx += 3;
    }
    if (!pack_lstm(h, "encoder.model.13", p, o.lstm)) return -1;
    if (!pack_conv(h, "encoder.model.15.conv.conv", kH, kDim, 7, p, o.fin)) return -1;
    if (int rc = pack_codebooks(h, p, o)) return rc;
    if (!with_decoder) return 0;
    if (!pack_conv(h, "decoder.model.0.conv.conv", kDim, kH, 7, p, o.dconv0)) return -1;
    if (!pack_lstm(h, "decoder.model.1", p, o.dlstm)) return -1;
    int Cd = kH, di = 3;
    for (int s = 0; s < 4; ++s) {
        if (!pack_convtr(h, "decoder.model." + std::to_string(di) + ".convtr.convtr", Cd, Cd / 2, kRatiosDec[s], p, o.dup[s])) return -1;
        Cd /= 2;
        if (!pack_block(h, "decoder.model." + std::to_string(di + 1), Cd, p, o.dres[s])) return -1;
        di += 3;
    }
    if (!pack_conv(h, "decoder.model.15.conv.conv", 32, 1, 7, p, o.dlast)) return -1;
    return 0;
}

void set_conv(ConvW& c, const float* blob, Off o, int cin, int cout, int k, int stride) {
    c.w = blob + o.w; c.b = blob + o.b; c.cin = cin; c.cout = cout; c.k = k; c.stride = stride;
}
void set_block(ConvW (&r)[3], const float* blob, const Off (&o)[3], int C) {
    set_conv(r[0], blob, o[0], C, C / 2, 3, 1);
    set_conv(r[1], blob, o[1], C / 2, C, 1, 1);
    set_conv(r[2], blob, o[2], C, C, 1, 1);
}

// the handle's fp32 weight pointers into the uploaded blob
void bind_weights(at_encodec* h, const Offsets& o, bool with_decoder) {
    const float* bl = h->blob;
    set_conv(h->conv0, bl, o.conv0, 1, 32, 7, 1);
    int C = 32;
    for (int s = 0; s < 4; ++s) {
        set_block(h->res[s], bl, o.res[s], C);
        set_conv(h->down[s], bl, o.down[s], C, 2 * C, 2 * kRatiosEnc[s], kRatiosEnc[s]);
        C *= 2;
    }
    set_conv(h->fin, bl, o.fin, kH, kDim, 7, 1);
    h->codebooks = bl + o.cb;
    h->e2 = bl + o.e2;
    h->n_codebooks = o.ncb;
    if (!with_decoder) return;
    set_conv(h->dconv0, bl, o.dconv0, kDim, kH, 7, 1);
    int Cd = kH;
    for (int s = 0; s < 4; ++s) {
        // transposed conv as a k=2, stride-1, zero-left-pad GEMM with N = s*Cout
        set_conv(h->dup[s], bl, o.dup[s], Cd, kRatiosDec[s] * (Cd / 2), 2, 1);
        Cd /= 2;
        set_block(h->dres[s], bl, o.dres[s], Cd);
    }
    set_conv(h->dlast, bl, o.dlast, 32, 1, 7, 1);
}

float max_abs(const std::vector<float>& host, size_t off, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::fmax(mx, std::fabs(host[off + i]));
    return mx;
}

// Device room for the pieces of an n-element weight whose host copy lies at host[off]: for the fp16 scheme two pieces and the power-of-two scale
// that puts max |w| into [2^14, 2^15), for the bf16 scheme three pieces and scale 1. The handle owns the allocation from here on.
int alloc_pieces(at_encodec* h, const std::vector<float>& host, size_t off, size_t n, int scheme, piece_t** d, SplitW& out) {
    out.s = scheme == XB_SCHEME_F16X2 ? xb_weight_scale(max_abs(host, off, n)) : 1.0f;
    *d = nullptr;
    AT_CHECK_HIP(hipMalloc((void**)d, (size_t)xb_pieces(scheme) * n * sizeof(piece_t)));
    h->extra_allocs.push_back(*d);
    out.p = *d;
    return 0;
}
// W [N][K] (device, fp32; host copy at host[off]) as K-blocked pieces of `scheme`; cblocks > 0: a packed conv weight of Cin = 16 * cblocks whose
// K-blocks go in the window order of a conv with `stride` (gemm_bf16x3.h, launch_split_blocked)
int pack_pieces(at_encodec* h, const std::vector<float>& host, size_t off, const float* w, int N, int K, int scheme, int cblocks, int stride, SplitW& out) {
    piece_t* d;
    if (int rc = alloc_pieces(h, host, off, (size_t)N * K, scheme, &d, out)) return rc;
    return launch_split_blocked(w, K, N, N, K, d, nullptr, scheme, out.s, nullptr, cblocks, stride);
}

// one LSTM: fp32 pointers and, with bf16x3, its input projections as operand pieces of both schemes and the W_hh scales of the fp16-scheme recurrence
int fill_lstm(at_encodec* h, LstmW& w, const std::vector<float>& host, const size_t off[2][4]) {
    for (int l = 0; l < 2; ++l) {
        w.wih[l] = h->blob + off[l][0]; w.whh[l] = h->blob + off[l][1]; w.bih[l] = h->blob + off[l][2]; w.bhh[l] = h->blob + off[l][3];
        if (!h->bf16x3) continue;
        SplitW s3, f2;
        if (int rc = pack_pieces(h, host, off[l][0], w.wih[l], 4 * kH, kH, XB_SCHEME_BF16X3, 0, 1, s3)) return rc;
        if (int rc = pack_pieces(h, host, off[l][0], w.wih[l], 4 * kH, kH, XB_SCHEME_F16X2, 0, 1, f2)) return rc;
        w.wih_s[l] = s3.p; w.wih_f[l] = f2.p; w.wih_fs[l] = f2.s;
        w.whh_fs[l] = xb_weight_scale(max_abs(host, off[l][1], (size_t)4 * kH * kH));
    }
    return 0;
}

// stage 0: Wsc . conv0 as one 7-tap conv of the waveform (float64 products, rounded once) for seanet_stage0x3.hip
int fold_stage0_shortcut(at_encodec* h, const std::vector<float>& host, const Offsets& o) {
    std::vector<float> f(32 * 7 + 32);
    const float* wt = host.data() + o.res[0][1].w;   // [32][16 + 32] = [W1 | Wsc]
    const float* bt = host.data() + o.res[0][1].b;   // b1 + bsc
    const float* w0 = host.data() + o.conv0.w;       // [32][7]
    const float* b0 = host.data() + o.conv0.b;
    for (int c = 0; c < 32; ++c) {
        for (int j = 0; j < 7; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 32; ++k) acc += (double)wt[c * 48 + 16 + k] * (double)w0[k * 7 + j];
            f[c * 7 + j] = (float)acc;
        }
        double accb = (double)bt[c];
        for (int k = 0; k < 32; ++k) accb += (double)wt[c * 48 + 16 + k] * (double)b0[k];
        f[32 * 7 + c] = (float)accb;
    }
    float* d = nullptr;
    AT_CHECK_HIP(hipMalloc((void**)&d, f.size() * sizeof(float)));
    h->extra_allocs.push_back(d);
    AT_CHECK_HIP(hipMemcpy(d, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    h->sc0_w = d;
    return 0;
}

// bf16x3, encoder side: the RVQ codebooks, the stage 2-3 GEMM chain and the final conv as pieces; the fused kernels' weight scales
int split_encoder(at_encodec* h, const std::vector<float>& host, const Offsets& o) {
    {   // codebooks as plain (row-major) bf16 pieces for the RVQ search, and as two fp16 pieces of E * 2^k (one power of two for all codebooks: the
        // order of the distances is untouched)
        const size_t n = (size_t)h->n_codebooks * kCodes * kDim;
        piece_t* d;
        SplitW s3;
        if (int rc = alloc_pieces(h, host, o.cb, n, XB_SCHEME_BF16X3, &d, s3)) return rc;
        if (int rc = launch_split_plain(h->codebooks, (long long)n, d, nullptr)) return rc;
        h->cb_s = s3.p;
        if (int rc = alloc_pieces(h, host, o.cb, n, XB_SCHEME_F16X2, &d, h->cb_f)) return rc;
        if (int rc = launch_split_plain(h->codebooks, (long long)n, d, nullptr, XB_SCHEME_F16X2, h->cb_f.s)) return rc;
    }
    // stage-2 strided conv [256][10 * 128], 256-channel block: conv3 [128][3 * 256] and tail [256][128 + 256] (a plain linear layer), stage-3 strided
    // conv [512][16 * 256]: as three bf16 pieces, and the same four as two fp16 pieces each scaled by its own power of two
    const ConvW* src[4] = {&h->down[2], &h->res[3][0], &h->res[3][1], &h->down[3]};
    const size_t off[4] = {o.down[2].w, o.res[3][0].w, o.res[3][1].w, o.down[3].w};
    const int ns[4] = {256, 128, 256, 512}, ks[4] = {1280, 768, 384, 4096};
    const int wcb[4] = {8, 16, 0, 16}, wst[4] = {5, 1, 1, 8};   // window description of the three convs
    const __bf16** s3[4] = {&h->down2_s, &h->res3c_s, &h->res3t_s, &h->down3_s};
    for (int j = 0; j < 4; ++j) {
        SplitW w3;
        if (int rc = pack_pieces(h, host, off[j], src[j]->w, ns[j], ks[j], XB_SCHEME_BF16X3, wcb[j], wst[j], w3)) return rc;
        *s3[j] = w3.p;
        if (int rc = pack_pieces(h, host, off[j], src[j]->w, ns[j], ks[j], XB_SCHEME_F16X2, wcb[j], wst[j], h->chain_f[j])) return rc;
    }
    // final conv [128][7 * 512]
    if (int rc = pack_pieces(h, host, o.fin.w, h->fin.w, kDim, 7 * kH, XB_SCHEME_F16X2, kH / 16, 1, h->fin_f)) return rc;
    if (int rc = fold_stage0_shortcut(h, host, o)) return rc;
    // power-of-two weight scales of the fused residual blocks' and strided convs' fp16 scheme (the kernels split their weights themselves, once per launch)
    int C = 32;
    for (int s = 0; s < 4; ++s) {
        h->res_fs[s][0] = xb_weight_scale(max_abs(host, o.res[s][0].w, (size_t)(C / 2) * 3 * C));
        h->res_fs[s][1] = xb_weight_scale(max_abs(host, o.res[s][1].w, (size_t)C * (C / 2 + C)));
        h->down_fs[s] = xb_weight_scale(max_abs(host, o.down[s].w, (size_t)2 * C * 2 * kRatiosEnc[s] * C));
        C *= 2;
    }
    return 0;
}

// bf16x3, decoder side: block scales, the stage-0 block and the transposed convs of stages 0-2 as two fp16 pieces
int split_decoder(at_encodec* h, const std::vector<float>& host, const Offsets& o) {
    int C = kH / 2;
    for (int s = 0; s < 4; ++s) {
        h->dres_fs[s][0] = xb_weight_scale(max_abs(host, o.dres[s][0].w, (size_t)(C / 2) * 3 * C));
        h->dres_fs[s][1] = xb_weight_scale(max_abs(host, o.dres[s][1].w, (size_t)C * (C / 2 + C)));
        if (s < 3) {   // transposed conv of this stage as a two-tap windowed split GEMM: [r * Cout][2 * Cin], Cin = 2 * C
            const int Cin = 2 * C, N = kRatiosDec[s] * C, K = 2 * Cin;
            if (N % 64 == 0 && K % 64 == 0)
                if (int rc = pack_pieces(h, host, o.dup[s].w, h->dup[s].w, N, K, XB_SCHEME_F16X2, Cin / 16, 1, h->dup_f[s])) return rc;
        }
        C /= 2;
    }
    // the 256-channel block's two weight matrices for the split GEMMs (as the encoder's chain_f[1], chain_f[2]); their scales are dres_fs[0]
    if (int rc = pack_pieces(h, host, o.dres[0][0].w, h->dres[0][0].w, 128, 768, XB_SCHEME_F16X2, 16, 1, h->dchain_f[0])) return rc;
    if (int rc = pack_pieces(h, host, o.dres[0][1].w, h->dres[0][1].w, 256, 384, XB_SCHEME_F16X2, 0, 1, h->dchain_f[1])) return rc;
    h->dtail_up_fs = xb_weight_scale(max_abs(host, o.dup[3].w, (size_t)64 * 128));   // the fused tail kernel's transposed conv [2 * 32][2 * 64]
    return 0;
}

// what the environment decides once per handle
int read_environment(at_encodec* h) {
    hipDeviceProp_t prop;
    AT_CHECK_HIP(hipGetDeviceProperties(&prop, h->device));
    const char* env = std::getenv("AUDIOTOKEN_LSTM_STEPWISE");
    h->opt.persistent_lstm = prop.multiProcessorCount >= 256 && !(env && env[0] == '1');
    const char* e = std::getenv("AUDIOTOKEN_BF16X3_ACOUSTIC");
    h->bf16x3 = e ? std::atoi(e) != 0 : kBf16x3AcousticDefault;
    // which fused SEANet kernels use the split-bf16 variants: bit 0 stage-1 strided conv, bit 1 128-channel block, bit 2 64-channel block, bit 3 stage 0, bit 4 / 5 stage-2 / stage-3 strided conv (GEMM), bit 6 256-channel block (GEMMs), bit 7 LSTM recurrence, bit 8 RVQ search
    const char* m = std::getenv("AUDIOTOKEN_X3_KERNELS");
    const int mask = m ? std::atoi(m) : 511;
    Options& o = h->opt;
    o.down64_x3 = (mask & 1) != 0; o.res128_x3 = (mask & 2) != 0; o.res64_x3 = (mask & 4) != 0; o.stage0_x3 = (mask & 8) != 0;
    o.down128_x3 = (mask & 16) != 0;
    o.down256_x3 = (mask & 32) != 0;
    o.res256_x3 = (mask & 64) != 0;
    o.lstm_x3 = (mask & 128) != 0;
    o.rvq_x3 = (mask & 256) != 0;
    return 0;
}

}  // namespace

extern "C" int at_encodec_finalize(at_encodec_t* h, int with_decoder) {
    AT_REQUIRE(h && !h->finalized, "bad handle");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    Packer p;
    Offsets o;
    if (int rc = pack_host(h, with_decoder != 0, p, o)) return rc;
    h->blob_floats = p.host.size();
    AT_CHECK_HIP(hipMalloc((void**)&h->blob, h->blob_floats * sizeof(float)));
    AT_CHECK_HIP(hipMemcpy(h->blob, p.host.data(), h->blob_floats * sizeof(float), hipMemcpyHostToDevice));
    bind_weights(h, o, with_decoder != 0);
    h->has_decoder = with_decoder != 0;
    if (int rc = read_environment(h)) return rc;
    h->staged.clear();
    if (int rc = fill_lstm(h, h->lstm, p.host, o.lstm)) return rc;
    if (with_decoder)
        if (int rc = fill_lstm(h, h->dlstm, p.host, o.dlstm)) return rc;
    if (h->bf16x3) {
        if (int rc = split_encoder(h, p.host, o)) return rc;
        if (with_decoder)
            if (int rc = split_decoder(h, p.host, o)) return rc;
        AT_CHECK_HIP(hipDeviceSynchronize());
    }
    if (!host_only_test()) {
        AT_CHECK_HIP(hipMalloc((void**)&h->range_tab, 64 * sizeof(int)));
        h->extra_allocs.push_back(h->range_tab);
        AT_CHECK_HIP(hipMemset(h->range_tab, 0, 64 * sizeof(int)));
    }
    h->finalized = true;
    return 0;
}
