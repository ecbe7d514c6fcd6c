// Acoustic tokenizer (EnCodec 24 kHz) — the C ABI of include/audiotoken_hip.h: handle lifecycle, options, profile and range reports, stream
// bookkeeping and the at_op_* operators. The handle is in encodec_handle.h, plans and routes in encodec_plan.h, weight intake in encodec_finalize.hip,
// the launch sequences in encodec_encode.hip / encodec_decode.hip / encodec_lstm.hip.
#include <cstring>

#include "encodec_handle.h"

namespace at {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
const char* last_error_cstr() { return g_last_error.c_str(); }

hipEvent_t Profiler::get_event() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
void Profiler::begin(const char* group, int launches, hipStream_t s) {
    if (!enabled) return;
    int g = -1;
    for (size_t i = 0; i < names.size(); ++i) if (names[i] == group) { g = (int)i; break; }
    if (g < 0) { names.push_back(group); g = (int)names.size() - 1; }
    Span sp{g, launches, get_event(), get_event()};
    (void)hipEventRecord(sp.a, s);
    spans.push_back(sp);
    open_ = (int)spans.size() - 1;
}
void Profiler::end(hipStream_t s) {
    if (!enabled || open_ < 0) return;
    (void)hipEventRecord(spans[open_].b, s);
    open_ = -1;
}
void Profiler::reset() {
    for (auto& sp : spans) { pool.push_back(sp.a); pool.push_back(sp.b); }
    spans.clear();
    names.clear();
    open_ = -1;
}
int Profiler::read(std::vector<float>& ms, std::vector<int>& launches) {
    ms.assign(names.size(), 0.f);
    launches.assign(names.size(), 0);
    for (auto& sp : spans) {
        if (hipEventSynchronize(sp.b) != hipSuccess) return -2;
        float t = 0.f;
        if (hipEventElapsedTime(&t, sp.a, sp.b) != hipSuccess) return -2;
        ms[sp.group] += t;
        launches[sp.group] += sp.launches;
    }
    return 0;
}
int Profiler::read_groups(char* names_out, size_t names_cap, float* total_ms, int* launches, int max_groups) {
    std::vector<float> ms;
    std::vector<int> ln;
    if (read(ms, ln) != 0) { set_error("profile read: event query failed"); return -2; }
    std::string joined;
    int n = 0;
    for (size_t i = 0; i < names.size() && n < max_groups; ++i, ++n) {
        joined += names[i];
        joined += '\n';
        total_ms[n] = ms[i];
        launches[n] = ln[i];
    }
    AT_REQUIRE(joined.size() + 1 <= names_cap, "names buffer too small");
    std::memcpy(names_out, joined.c_str(), joined.size() + 1);
    return n;
}
Profiler::~Profiler() {
    reset();
    for (auto e : pool) (void)hipEventDestroy(e);
}

static const char* const kAcSiteNames[AC_NSITES] = {"stage0", "res1", "down1", "res2", "down2", "res3_conv", "res3_tail", "lstm_ih", "final_conv_in", "rvq",
                                                   "dec_lstm_ih", "dec_up", "dec_res"};
// status word of the *_checked entry points: bit 0 = an LSTM hand-off wait gave up (sync[63]), bit 1 = fp16 range overflow at any site, bit 2 = a NaN /
// infinity reached the RVQ search (XB_STATUS_NONFINITE)
__global__ void status_combine_kernel(const unsigned* sync, const int* range_tab, int nsites, unsigned* out) {
    unsigned v = sync[63] ? 1u : 0u;
    for (int k = 0; k < nsites; ++k) v |= (unsigned)range_tab[2 * k] & (unsigned)(XB_STATUS_F16_OVERFLOW | XB_STATUS_NONFINITE);
    out[0] = v;
}
int launch_status_combine(const unsigned* sync, const int* range_tab, unsigned* out, hipStream_t stream) {
    hipLaunchKernelGGL(status_combine_kernel, dim3(1), dim3(1), 0, stream, sync, range_tab, (int)AC_NSITES, out);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace at

using namespace at;

extern "C" {

int at_version(void) { return 1; }
const char* at_last_error(void) { return at::last_error_cstr(); }

at_encodec_t* at_encodec_create(int device_id) {
    if (!device_exists("at_encodec_create", device_id)) return nullptr;
    at_encodec* h = new at_encodec();
    h->device = device_id;
    return h;
}
int at_encodec_set_tensor(at_encodec_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    return stage_tensor(h, name, host_data, shape, ndim);
}

void at_encodec_destroy(at_encodec_t* h) {
    if (!h) return;
    DeviceGuard guard(h->device);   // restores the caller's current device (destroy runs from garbage collection in Python)
    if (h->blob) (void)hipFree(h->blob);
    for (void* p : h->extra_allocs) (void)hipFree(p);
    delete h;
}

int at_encodec_num_codebooks(const at_encodec_t* h) { return h ? h->n_codebooks : 0; }

size_t at_encodec_workspace_bytes(const at_encodec_t* h, int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return make_plan(B, N, h ? h->sub_batch : sub_batch()).total_floats * sizeof(float);
}

int at_encodec_encode(at_encodec_t* h, const float* wav, const float* mask, int B, int N, int n_q, int16_t* codes, int* T_out,
                      float* emb_out, void* workspace, size_t workspace_bytes, at_stream_t stream) {
    (void)mask;  // the reference's AcousticEncoder.forward ignores attention_mask (audiotoken/encoder.py:44-52)
    return encodec_encode_impl(h, wav, B, N, n_q, codes, T_out, emb_out, workspace, workspace_bytes, stream, nullptr, nullptr);
}

int at_encodec_encode_checked(at_encodec_t* h, const float* wav, const float* mask, int B, int N, int n_q, int16_t* codes, int* T_out,
                              float* emb_out, void* workspace, size_t workspace_bytes, at_stream_t stream, uint32_t* status_dev) {
    (void)mask;
    return encodec_encode_impl(h, wav, B, N, n_q, codes, T_out, emb_out, workspace, workspace_bytes, stream, status_dev, nullptr);
}

size_t at_encodec_stream_state_bytes(const at_encodec_t* h, int B) {
    (void)h;
    return B >= 1 ? StreamState::floats(B) * sizeof(float) : 0;
}

int at_encodec_stream_reset(at_encodec_t* h, void* state_dev, int B, at_stream_t stream) {
    AT_REQUIRE(h && h->finalized, "model not finalized");
    AT_REQUIRE(state_dev && B >= 1, "at_encodec_stream_reset: null state or B < 1");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_CHECK_HIP(hipMemsetAsync(state_dev, 0, StreamState::floats(B) * sizeof(float), (hipStream_t)stream));   // h = c = 0
    at_encodec::StreamInfo info;
    info.B = B;
    h->streams[state_dev] = info;
    return 0;
}

size_t at_encodec_stream_workspace_bytes(const at_encodec_t* h, int B, int n_new) {
    if (B <= 0 || n_new <= 0) return 0;
    const int sub = h ? h->sub_batch : sub_batch();
    const size_t a = make_stream_plan(B, n_new, true, sub).total_floats, b = make_stream_plan(B, n_new, false, sub).total_floats;
    return (a > b ? a : b) * sizeof(float);
}

int at_encodec_encode_stream_checked(at_encodec_t* h, const void* state_in, void* state_out, const float* wav_new, int B, int n_new, int final,
                                     int n_q, int16_t* codes, int* T_out, float* emb_out, void* workspace, size_t workspace_bytes,
                                     at_stream_t stream, uint32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "model not finalized");
    AT_REQUIRE(state_in && state_out, "at_encodec_encode_stream_checked: null state");
    AT_REQUIRE(state_in != state_out, "at_encodec_encode_stream_checked: state_in and state_out must be two buffers (a failed push is repeated from state_in)");
    AT_REQUIRE(B >= 1 && n_new >= 0, "at_encodec_encode_stream_checked: need B >= 1 and n_new >= 0");
    const auto it = h->streams.find(state_in);
    AT_REQUIRE(it != h->streams.end(), "at_encodec_encode_stream_checked: state_in was neither reset (at_encodec_stream_reset) nor written by a push of this handle");
    const at_encodec::StreamInfo in = it->second;
    AT_REQUIRE(!in.decode, "at_encodec_encode_stream_checked: state_in is a decode stream's state (at_encodec_decode_stream_reset)");
    AT_REQUIRE(in.B == B, "at_encodec_encode_stream_checked: the state was reset for another B");
    AT_REQUIRE(!in.finished, "at_encodec_encode_stream_checked: push after the final push (reset the stream first)");
    AT_REQUIRE(final || (n_new > 0 && n_new % kHop == 0), "at_encodec_encode_stream_checked: n_new must be a positive multiple of 320 unless final");
    AT_REQUIRE(final || in.started || n_new >= kStreamFirstFrames * kHop, "at_encodec_encode_stream_checked: the first push of a stream needs at least 7 frames (2240 samples) unless final");
    at_encodec::StreamInfo out = in;
    out.started = true;
    out.finished = final != 0;
    if (n_new == 0) {   // a final push without samples: the stream ends on a frame boundary, nothing is left to emit
        if (T_out) *T_out = 0;
        if (status_dev) AT_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(uint32_t), (hipStream_t)stream));
        h->streams[state_out] = out;
        return 0;
    }
    const StreamCall sc{state_in, state_out, in.started, final != 0};
    int T = 0;
    if (int rc = encodec_encode_impl(h, wav_new, B, n_new, n_q, codes, &T, emb_out, workspace, workspace_bytes, stream, status_dev, &sc)) return rc;
    if (T_out) *T_out = T;
    h->streams[state_out] = out;
    return 0;
}

namespace {
struct BoolOption { const char* name; bool Options::*member; };
const BoolOption kBoolOptions[] = {
    {"dec_skip_twin", &Options::dec_skip_twin},
    {"persistent_lstm", &Options::persistent_lstm},
    {"fused_stage0", &Options::fused_stage0},
    {"fused_res64", &Options::fused_res64},
    {"fused_res128", &Options::fused_res128},
    {"fused_down64", &Options::fused_down64},
    {"fused_stage1", &Options::fused_stage1},
    {"down64_x3", &Options::down64_x3},
    {"rvq_x3", &Options::rvq_x3},
    {"lstm_x3", &Options::lstm_x3},
    {"res256_x3", &Options::res256_x3},
    {"down256_x3", &Options::down256_x3},
    {"down128_x3", &Options::down128_x3},
    {"stage0_x3", &Options::stage0_x3},
    {"res64_x3", &Options::res64_x3},
    {"res128_x3", &Options::res128_x3},
    {"fused_dectail", &Options::fused_dectail},
    {"tail_f16x2", &Options::tail_f16x2},
    {"dec_chain", &Options::dec_chain},
    {"ih_f16x2", &Options::ih_f16x2},
    {"res_f16x2", &Options::res_f16x2},
    {"rvq_f16x2", &Options::rvq_f16x2},
    {"fin_f16x2", &Options::fin_f16x2},
    {"res128_rs", &Options::res128_rs},
    {"up_f16x2", &Options::up_f16x2},
    {"lstm_f16x2", &Options::lstm_f16x2},
    {"lstm_pipe", &Options::lstm_pipe},
    {"chain_f16x2", &Options::chain_f16x2},
};
}  // namespace

int at_encodec_set_option(at_encodec_t* h, const char* name, int value) {
    AT_REQUIRE(h && name, "null pointer");
    const std::string n(name);
    for (const BoolOption& o : kBoolOptions)
        if (n == o.name) { h->opt.*(o.member) = value != 0; return 0; }
    if (n == "lstm_spin_limit") { AT_REQUIRE(value >= 0, "lstm_spin_limit must be >= 0"); h->lstm_spin_limit = (unsigned)value; return 0; }
    if (n == "subbatch") { AT_REQUIRE(value >= 1, "subbatch must be >= 1"); h->sub_batch = value; return 0; }
    set_error(std::string("unknown option ") + name);
    return -1;
}

int at_encodec_get_option(const at_encodec_t* h, const char* name) {
    if (!h || !name) return -1;
    const std::string n(name);
    for (const BoolOption& o : kBoolOptions)
        if (n == o.name) return h->opt.*(o.member) ? 1 : 0;
    if (n == "lstm_spin_limit") return (int)h->lstm_spin_limit;
    if (n == "subbatch") return h->sub_batch;
    return -1;
}

// The measured fp16 headroom of the LAST encode / decode call of this handle: for every site (at_encodec_range_sites) the largest |x * scale| a
// split writer saw, 0 for sites that did not run on the fp16 scheme; the scheme overflows at 65504. Synchronises the device.
int at_encodec_range_report(at_encodec_t* h, float* max_scaled, int cap) {
    AT_REQUIRE(h && h->finalized && h->range_tab && max_scaled && cap >= (int)AC_NSITES, "at_encodec_range_report: bad arguments");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    int host[2 * AC_NSITES];
    AT_CHECK_HIP(hipDeviceSynchronize());
    AT_CHECK_HIP(hipMemcpy(host, h->range_tab, sizeof(host), hipMemcpyDeviceToHost));
    for (int k = 0; k < (int)AC_NSITES; ++k) { float f; std::memcpy(&f, &host[2 * k + 1], sizeof(f)); max_scaled[k] = f; }
    return (int)AC_NSITES;
}
int at_encodec_range_sites(char* names, size_t cap) {
    std::string s;
    for (int k = 0; k < (int)AC_NSITES; ++k) { s += kAcSiteNames[k]; s += "\n"; }
    if (!names || cap < s.size() + 1) return -(int)(s.size() + 1);
    std::memcpy(names, s.c_str(), s.size() + 1);
    return (int)AC_NSITES;
}

int at_encodec_profile(at_encodec_t* h, int enable) { return profile_enable(h, enable); }
int at_encodec_profile_read(at_encodec_t* h, char* names, size_t names_cap, float* total_ms, int* launches, int max_groups) {
    return profile_read(h, names, names_cap, total_ms, launches, max_groups);
}

size_t at_encodec_decode_workspace_bytes(const at_encodec_t* h, int B, int T) {
    if (B <= 0 || T <= 0) return 0;
    return make_dec_plan(B, T, h ? h->sub_batch : sub_batch()).total_floats * sizeof(float);
}

int at_encodec_decode(at_encodec_t* h, const int64_t* codes, int B, int K, int T, float* wav, void* workspace,
                      size_t workspace_bytes, at_stream_t stream_) {
    return at_encodec_decode_checked(h, codes, B, K, T, wav, workspace, workspace_bytes, stream_, nullptr);
}

int at_encodec_decode_checked(at_encodec_t* h, const int64_t* codes, int B, int K, int T, float* wav, void* workspace,
                              size_t workspace_bytes, at_stream_t stream_, uint32_t* status_dev) {
    return encodec_decode_impl(h, codes, B, K, T, wav, workspace, workspace_bytes, stream_, status_dev, nullptr);
}

size_t at_encodec_decode_stream_state_bytes(const at_encodec_t* h, int B) {
    (void)h;
    return B >= 1 ? DecStreamState::floats(B) * sizeof(float) : 0;
}

int at_encodec_decode_stream_reset(at_encodec_t* h, void* state_dev, int B, at_stream_t stream) {
    AT_REQUIRE(h && h->finalized && h->has_decoder, "model not finalized with a decoder");
    AT_REQUIRE(state_dev && B >= 1, "at_encodec_decode_stream_reset: null state or B < 1");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_CHECK_HIP(hipMemsetAsync(state_dev, 0, DecStreamState::floats(B) * sizeof(float), (hipStream_t)stream));   // h = c = 0
    at_encodec::StreamInfo info;
    info.B = B;
    info.decode = true;
    h->streams[state_dev] = info;
    return 0;
}

size_t at_encodec_decode_stream_workspace_bytes(const at_encodec_t* h, int B, int t_new) {
    if (B <= 0 || t_new <= 0) return 0;
    const int sub = h ? h->sub_batch : sub_batch();
    const size_t a = make_dec_stream_plan(B, t_new, true, sub).total_floats, b = make_dec_stream_plan(B, t_new, false, sub).total_floats;
    return (a > b ? a : b) * sizeof(float);
}

int at_encodec_decode_stream_checked(at_encodec_t* h, const void* state_in, void* state_out, const int64_t* codes_new, int B, int K, int t_new,
                                     float* wav_out, void* workspace, size_t workspace_bytes, at_stream_t stream, uint32_t* status_dev) {
    AT_REQUIRE(h && h->finalized && h->has_decoder, "model not finalized with a decoder");
    AT_REQUIRE(state_in && state_out, "at_encodec_decode_stream_checked: null state");
    AT_REQUIRE(state_in != state_out, "at_encodec_decode_stream_checked: state_in and state_out must be two buffers (a failed push is repeated from state_in)");
    AT_REQUIRE(B >= 1 && t_new >= 1, "at_encodec_decode_stream_checked: need B >= 1 and t_new >= 1");
    const auto it = h->streams.find(state_in);
    AT_REQUIRE(it != h->streams.end(), "at_encodec_decode_stream_checked: state_in was neither reset (at_encodec_decode_stream_reset) nor written by a push of this handle");
    const at_encodec::StreamInfo in = it->second;
    AT_REQUIRE(in.decode, "at_encodec_decode_stream_checked: state_in is an encode stream's state (at_encodec_stream_reset)");
    AT_REQUIRE(in.B == B, "at_encodec_decode_stream_checked: the state was reset for another B");
    AT_REQUIRE(in.started || t_new >= kDecFirstFrames, "at_encodec_decode_stream_checked: the first push of a stream needs at least 7 frames");
    const DecStreamCall sc{state_in, state_out, in.started};
    if (int rc = encodec_decode_impl(h, codes_new, B, K, t_new, wav_out, workspace, workspace_bytes, stream, status_dev, &sc)) return rc;
    at_encodec::StreamInfo out = in;
    out.started = true;
    h->streams[state_out] = out;
    return 0;
}

// Stream pools (stream_pool.hip): rows of a state moved between a pool of S slots and a staging state of B rows. Everything is checked on the host,
// from the caller's host copy of the slot list, before the device is touched.
namespace {
const int kEncPlaneWidths[] = {kStreamCtx, kH, kH, kH, kH, kStreamHist * kH};   // StreamState: ctx, h0, c0, h1, c1, yhist
const int kDecPlaneWidths[] = {kDecHist * kDim, kH, kH, kH, kH, kDecCtx * kH};  // DecStreamState: zhist, h0, c0, h1, c1, yctx

int stream_pool_copy(at_encodec_t* h, bool decode, bool gather, const void* pool, int S, const void* state, int B, const int32_t* slots_dev,
                     const int32_t* slots_host, at_stream_t stream) {
    AT_REQUIRE(h && h->finalized && (!decode || h->has_decoder), decode ? "model not finalized with a decoder" : "model not finalized");
    AT_REQUIRE(pool && state && slots_dev && slots_host, "stream pool: null pool, state or slot list");
    AT_REQUIRE(pool != state, "stream pool: the staging state and the pool must be two buffers");
    AT_REQUIRE(B >= 1 && B <= S, "stream pool: need 1 <= B <= S");
    const auto pit = h->streams.find(pool);
    AT_REQUIRE(pit != h->streams.end() && pit->second.B == S && pit->second.decode == decode,
               "stream pool: the pool was not reset for S streams of this direction by this handle (at_encodec_stream_reset / at_encodec_decode_stream_reset)");
    at_encodec::StreamInfo note;
    if (!gather) {
        const auto sit = h->streams.find(state);
        AT_REQUIRE(sit != h->streams.end(), "stream pool: state_in was neither reset nor written by a push or a gather of this handle");
        note = sit->second;
        AT_REQUIRE(note.B == B && note.decode == decode, "stream pool: state_in is a state of another B or direction");
        AT_REQUIRE(!note.finished, "stream pool: state_in is a finished stream's state");
    }
    if (int rc = check_pool_slots(slots_host, B, S)) return rc;
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    const int* widths = decode ? kDecPlaneWidths : kEncPlaneWidths;
    if (int rc = launch_stream_pool_copy(gather ? pool : state, const_cast<void*>(gather ? state : pool), slots_dev, widths, 6, B, S, gather, (hipStream_t)stream)) return rc;
    if (gather) {   // the staging state now holds B streams in mid-stream: the push accepts it as such
        note.B = B;
        note.started = true;
        note.decode = decode;
        h->streams[state] = note;
    }
    return 0;
}
}  // namespace

int at_encodec_stream_gather(at_encodec_t* h, const void* pool, int S, const int32_t* slots_dev, const int32_t* slots_host, int B, void* state_out,
                             at_stream_t stream) {
    return stream_pool_copy(h, false, true, pool, S, state_out, B, slots_dev, slots_host, stream);
}
int at_encodec_stream_scatter(at_encodec_t* h, const void* state_in, int B, const int32_t* slots_dev, const int32_t* slots_host, void* pool, int S,
                              at_stream_t stream) {
    return stream_pool_copy(h, false, false, pool, S, state_in, B, slots_dev, slots_host, stream);
}
int at_encodec_decode_stream_gather(at_encodec_t* h, const void* pool, int S, const int32_t* slots_dev, const int32_t* slots_host, int B, void* state_out,
                                    at_stream_t stream) {
    return stream_pool_copy(h, true, true, pool, S, state_out, B, slots_dev, slots_host, stream);
}
int at_encodec_decode_stream_scatter(at_encodec_t* h, const void* state_in, int B, const int32_t* slots_dev, const int32_t* slots_host, void* pool, int S,
                                     at_stream_t stream) {
    return stream_pool_copy(h, true, false, pool, S, state_in, B, slots_dev, slots_host, stream);
}

static GemmArgs gemm_args_of(const at_gemm_desc* d, const float* X2, int64_t x2_bstride, int ld2, int K1) {
    GemmArgs a;
    a.X = d->X; a.x_bstride = d->x_bstride; a.Tin = d->Tin; a.Cin = d->Cin; a.ldx = d->ldx;
    a.ktaps = d->ktaps; a.stride = d->stride; a.pad_left = d->pad_left; a.pad_mode = d->pad_mode;
    a.W = d->W; a.bias = d->bias; a.C = d->C; a.c_bstride = d->c_bstride; a.ldc = d->ldc;
    a.R = d->R; a.r_bstride = d->r_bstride; a.ldr = d->ldr;
    a.M = d->M; a.N = d->N; a.K = d->K; a.batch = d->batch; a.pro = d->pro; a.epi = d->epi; a.alpha = d->alpha;
    a.aux_off = d->aux_off; a.row_mask = d->row_mask;
    if (X2) { a.X2 = X2; a.x2_bstride = x2_bstride; a.ld2 = ld2; a.K1 = K1; }
    return a;
}

int at_op_gemm(const at_gemm_desc* d, at_stream_t stream) {
    AT_REQUIRE(d != nullptr, "null descriptor");
    return launch_gemm(gemm_args_of(d, nullptr, 0, 0, 0), (hipStream_t)stream);
}

int at_op_gemm_dual(const at_gemm_desc* d, const float* X2, int64_t x2_bstride, int ld2, int K1, at_stream_t stream) {
    AT_REQUIRE(d != nullptr, "null descriptor");
    AT_REQUIRE(X2 != nullptr, "at_op_gemm_dual: null second source (at_op_gemm is the single-source call)");
    return launch_gemm(gemm_args_of(d, X2, x2_bstride, ld2, K1), (hipStream_t)stream);
}

int at_op_gemm_route(const at_gemm_desc* d, const float* X2, int64_t x2_bstride, int ld2, int K1, int32_t* out) {
    AT_REQUIRE(d != nullptr && out != nullptr, "null descriptor or output");
    GemmRoute r;
    if (int rc = gemm_route(gemm_args_of(d, X2, x2_bstride, ld2, K1), r)) return rc;
    out[0] = r.config;
    for (int i = 0; i < 3; ++i) out[1 + i] = (int32_t)r.workgroups[i];
    return 0;
}

int at_op_rvq_encode(const float* x, int64_t rows, int T, const float* codebooks, const float* e2, int n_q, int16_t* codes,
                     at_stream_t stream) {
    AT_REQUIRE(x && codebooks && e2 && codes && T >= 1 && n_q >= 1, "bad arguments");
    return launch_rvq_encode(x, rows, T, codebooks, e2, n_q, codes, (hipStream_t)stream);
}

// The RVQ search with split dot products (rvq_encode_x3.hip) — what the product runs: scheme 1 = two fp16 pieces / three products (default, option
// "rvq_f16x2"), 0 = three bf16 pieces / six products (its range fallback). The codebooks are split into `workspace` first, as finalize() does.
int at_op_rvq_encode_split(const float* x, int64_t rows, int T, const float* codebooks, const float* e2, int n_q, int16_t* codes, int scheme,
                           float cb_max_abs, void* workspace, size_t workspace_bytes, int32_t* status_dev, at_stream_t stream_) {
    using namespace at;
    AT_REQUIRE(x && codebooks && e2 && codes && workspace && T >= 1 && n_q >= 1, "at_op_rvq_encode_split: bad arguments");
    AT_REQUIRE(scheme == XB_SCHEME_BF16X3 || scheme == XB_SCHEME_F16X2, "at_op_rvq_encode_split: scheme 0 (bf16x3) or 1 (f16x2)");
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = (long long)n_q * kCodes * kDim;
    const int np = xb_pieces(scheme);
    AT_REQUIRE(workspace_bytes >= (size_t)np * n * sizeof(piece_t) + 2 * sizeof(int), "at_op_rvq_encode_split: workspace too small (pieces * n_q * 1024 * 128 * 2 + 8 bytes)");
    __bf16* pieces = reinterpret_cast<__bf16*>(workspace);
    int* pair = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + (size_t)np * n * sizeof(piece_t));   // {flag, census} of this call
    const float cs = scheme == XB_SCHEME_F16X2 ? xb_weight_scale(cb_max_abs) : 1.0f;
    AT_CHECK_HIP(hipMemsetAsync(pair, 0, 2 * sizeof(int), stream));
    if (status_dev) AT_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    if (int rc = launch_split_plain(codebooks, n, pieces, stream, scheme, cs)) return rc;
    if (int rc = launch_rvq_encode_x3(x, rows, T, codebooks, pieces, n, e2, n_q, codes, stream, scheme, scheme == XB_SCHEME_F16X2 ? XB_F16_ACT_SCALE : 1.0f, cs, pair)) return rc;
    return launch_range_combine(pair, 1, reinterpret_cast<int*>(status_dev), stream);
}

}  // extern "C"
