// The argument checks of the sampler's truncation (audiotoken_amd/csrc/gpt.hip: at_gpt_set_truncation; gpt_model.hip: at_op_nucleus_sample)
// under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program. Every refused case is refused before anything is launched and the accepted
// ones only write the handle, so it needs no device: the handle is a finalized at_gpt built by hand (decoder_args_common.h). Built and run by
// `make -C audiotoken_amd/csrc gpt_nucleus_asan`.
#include "decoder_args_common.h"

int main() {
    at_gpt model;
    finalize_by_hand(&model, 128);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");

    // ---- at_gpt_set_truncation
    expect(model.top_p == 1.0f && model.lmin == -inf, "a new handle has both cuts off");
    auto set = [&](at_gpt* h, float p, float q) {
        at::g_error.clear();
        return at_gpt_set_truncation(h, p, q);
    };
    expect(refused(set(nullptr, 0.9f, 0.0f), "null handle"), "set: a null handle");
    expect(set(&model, 0.9f, 0.05f) == 0 && model.top_p == 0.9f, "set: top_p 0.9, min_p 0.05");
    expect(model.lmin == (float)std::log((double)0.05f), "set: lmin is the double logarithm of the fp32 min_p, rounded once");
    const float p0 = model.top_p, l0 = model.lmin;
    struct Bad { float p, q; const char* text; const char* what; };
    const Bad bad[] = {
        {0.0f, 0.0f, "top_p must lie in (0, 1]", "top_p = 0"},
        {-0.5f, 0.0f, "top_p must lie in (0, 1]", "top_p < 0"},
        {1.0f + 1e-6f, 0.0f, "top_p must lie in (0, 1]", "top_p just above 1"},
        {inf, 0.0f, "top_p must lie in (0, 1]", "top_p = inf"},
        {nan, 0.0f, "top_p must lie in (0, 1]", "top_p = NaN"},
        {0.9f, 1.0f, "min_p must lie in [0, 1)", "min_p = 1"},
        {0.9f, -1e-6f, "min_p must lie in [0, 1)", "min_p < 0"},
        {0.9f, inf, "min_p must lie in [0, 1)", "min_p = inf"},
        {0.9f, nan, "min_p must lie in [0, 1)", "min_p = NaN"},
        {nan, nan, "top_p must lie in (0, 1]", "both NaN"},
    };
    for (const Bad& b : bad) {
        expect(refused(set(&model, b.p, b.q), b.text), b.what);
        expect(model.top_p == p0 && model.lmin == l0, "a refused call leaves the handle as it was");
    }
    expect(set(&model, std::numeric_limits<float>::denorm_min(), 0.0f) == 0 && model.lmin == -inf, "set: the smallest top_p; min_p 0 is off");
    expect(set(&model, 1.0f, std::numeric_limits<float>::denorm_min()) == 0 && model.top_p == 1.0f && std::isfinite(model.lmin), "set: top_p 1 is off; the smallest min_p");
    expect(set(&model, 1.0f, std::nextafterf(1.0f, 0.0f)) == 0 && model.lmin < 0.0f, "set: the largest min_p below 1");
    expect(set(&model, 1.0f, 0.0f) == 0 && model.top_p == 1.0f && model.lmin == -inf, "set: both off again");

    // ---- at_op_nucleus_sample
    auto sample = [&](const float* z, int B, int V, float t, int k, float p, float q, const float* u, std::vector<int32_t> allow, int32_t* out) {
        const auto a = exact_copy(allow);
        at::g_error.clear();
        return at_op_nucleus_sample(z, B, V, t, k, p, q, u, a.get(), out, nullptr, nullptr, nullptr);
    };
    expect(refused(sample(nullptr, 1, 128, 1.f, 1, 0.9f, 0.f, fake_f, {}, fake_i), "null pointer"), "sample: null logits");
    expect(refused(sample(fake_f, 1, 128, 1.f, 1, 0.9f, 0.f, nullptr, {}, fake_i), "null pointer"), "sample: null uniforms");
    expect(refused(sample(fake_f, 1, 128, 1.f, 1, 0.9f, 0.f, fake_f, {}, nullptr), "null pointer"), "sample: null out");
    expect(refused(sample(fake_f, 0, 128, 1.f, 1, 0.9f, 0.f, fake_f, {}, fake_i), "B must be"), "sample: B = 0");
    expect(refused(sample(fake_f, 65536, 128, 1.f, 1, 0.9f, 0.f, fake_f, {}, fake_i), "B must be"), "sample: B = 65536");
    expect(refused(sample(fake_f, 1, 0, 1.f, 1, 0.9f, 0.f, fake_f, {}, fake_i), "V must be"), "sample: V = 0");
    expect(refused(sample(fake_f, 1, 65537, 1.f, 1, 0.9f, 0.f, fake_f, {}, fake_i), "V must be"), "sample: V = 65537");
    expect(refused(sample(fake_f, 1, 128, 0.f, 1, 0.9f, 0.f, fake_f, {}, fake_i), "temperature"), "sample: temperature = 0");
    expect(refused(sample(fake_f, 1, 128, 1.f, 0, 0.9f, 0.f, fake_f, {}, fake_i), "top_k"), "sample: top_k = 0");
    for (const Bad& b : bad) expect(refused(sample(fake_f, 1, 128, 1.f, 1, b.p, b.q, fake_f, {}, fake_i), b.text), b.what);
    expect(refused(sample(fake_f, 1, 128, 1.f, 1, 0.9f, 0.f, fake_f, {0, 129, 0, 0}, fake_i), "allow ranges"), "sample: an allow range past V");
    expect(refused(sample(fake_f, 1, 128, 1.f, 1, 0.9f, 0.f, fake_f, {3, 3, 9, 9}, fake_i), "both empty"), "sample: allow ranges that allow nothing");
    return verdict("gpt nucleus argument checks");
}
