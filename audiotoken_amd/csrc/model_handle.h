// What the handles of the two semantic decoders (at_gpt in gpt.h, at_fine in fine.h) have in common, stated once: the staged host tensors, their upload with
// a shape check, the device allocations of finalize(), and the carver of a caller-owned state. Header-only, so the stand-alone argument checks (tools/) link
// nothing for it. HostTensor and device_exists also serve the tokenizers' handles (semantic_handle.h, encodec_handle.h).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "at_common.h"

namespace at {

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

// at_*_create: whether `device_id` names a HIP device; if not, the error is set in the name of the exported function `fn`
inline bool device_exists(const char* fn, int device_id) {
    int n = 0;
    if (!host_only_test() && (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n)) {
        set_error(std::string(fn) + ": no such HIP device " + std::to_string(device_id));
        return false;
    }
    return true;
}

// The fields the tools' hand-finalized handles and the entry points rely on, under these names
struct ModelHandle {
    int device = 0;
    bool finalized = false;
    std::map<std::string, HostTensor> staged;   // until finalize()
    std::vector<void*> allocs;                  // every device allocation of finalize()
};

// at_*_set_tensor: one host tensor copied into h->staged
inline int stage_model_tensor(ModelHandle* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    AT_REQUIRE(h && name && host_data && shape && ndim >= 1 && ndim <= 4, "bad arguments");
    AT_REQUIRE(!h->finalized, "model already finalized");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        AT_REQUIRE(shape[i] >= 1 && shape[i] <= (int64_t)1 << 32, "bad dimension");
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(host_data, host_data + n);
    h->staged[name] = std::move(t);
    return 0;
}

inline const HostTensor* staged_tensor(const ModelHandle* h, const std::string& name) {
    auto it = h->staged.find(name);
    return it == h->staged.end() ? nullptr : &it->second;
}

// the staged tensor `name` of exactly `shape` into its own device allocation; `fn` is the exported function the error texts name
inline int upload_staged(ModelHandle* h, const char* fn, const std::string& name, const std::vector<int64_t>& shape, const float** dst) {
    const HostTensor* t = staged_tensor(h, name);
    if (!t) { set_error(std::string(fn) + ": missing tensor " + name); return -1; }
    if (t->shape != shape) { set_error(std::string(fn) + ": tensor " + name + " has an unexpected shape"); return -1; }
    void* d = nullptr;
    AT_CHECK_HIP(hipMalloc(&d, t->data.size() * sizeof(float)));
    h->allocs.push_back(d);
    AT_CHECK_HIP(hipMemcpy(d, t->data.data(), t->data.size() * sizeof(float), hipMemcpyHostToDevice));
    *dst = static_cast<const float*>(d);
    return 0;
}

inline void free_allocs(ModelHandle* h) {
    for (void* p : h->allocs) (void)hipFree(p);
    h->allocs.clear();
}

// A caller-owned state cut into buffers, in the order they are taken, each rounded up to 256 bytes. A null base gives null buffers and the size alone.
struct StateCarver {
    char* base;
    size_t off;
    explicit StateCarver(void* base_, size_t off_ = 0) : base(static_cast<char*>(base_)), off(off_) {}
    template <class T>
    T* take(size_t count) {
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) / 256 * 256;
        return r;
    }
};

}  // namespace at
