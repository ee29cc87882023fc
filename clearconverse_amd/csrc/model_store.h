// model_store.h -- host-side weight staging and device allocation shared by every libccx handle that owns device memory
// (ccx_whisper, ccx_sepformer, ccx_speaker, ccx_resnet, ccx_specgate).  Host-only: no kernels, no launches.
//
// A handle embeds one ccx_dev_store by value.  set_tensor calls stage() the caller's tensors into host memory by name; finalize
// looks them up with need() (CCX_NEED), lays them out as its kernels want and upload()s them; destroy calls free_all().
#pragma once
#include <map>
#include <string>
#include <vector>
#include "../../include/ccx.h"
#include "ccx_common.h"

struct ccx_host_tensor {
  std::vector<float> data;
  std::vector<int64_t> shape;   // empty when the handle's set_tensor passes an element count only
};

inline float ccx_host_half_to_f32(uint16_t h) {
  const uint32_t s = (h >> 15) & 1, e = (h >> 10) & 0x1f, m = h & 0x3ff;
  uint32_t u;
  if (e == 0) {
    if (m == 0) u = s << 31;
    else {
      int ee = -1; uint32_t mm = m;
      do { ee++; mm <<= 1; } while (!(mm & 0x400));
      u = (s << 31) | ((uint32_t)(127 - 15 - ee) << 23) | ((mm & 0x3ff) << 13);
    }
  } else if (e == 31) u = (s << 31) | 0x7f800000u | (m << 13);
  else u = (s << 31) | ((e + 112) << 23) | (m << 13);
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct ccx_dev_store {
  ccx_ctx* ctx = nullptr;
  const char* model;            // prefix of every message: "whisper", "sepformer", "speaker", "resnet", "specgate"
  std::map<std::string, ccx_host_tensor> staged;
  std::vector<void*> allocs;    // every hipMalloc of the handle, freed by free_all()
  // Optional bump arena (open_arena): allocations are carved from ONE large hipMalloc in call order while they fit.
  char* arena = nullptr;
  size_t arena_cap = 0, arena_off = 0;
  // upload() zeroes the whole 256-byte-aligned block before the copy.  Kernels read past the logical end of several weight
  // buffers (the `+ 1024` / `+ slack` sizes in speaker.hip and resnet.hip), so only a handle whose kernels never do may clear this.
  bool zero_uploads = true;

  explicit ccx_dev_store(const char* model_tag) : model(model_tag) {}

  // ---- staging (set_tensor) ----
  // `shape` dims must be positive; f16 / bf16 data is widened to f32.  `data` may be host or device memory.
  int stage(const char* name, const void* data, int dtype, int ndim, const int64_t* shape) {
    ccx_host_tensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; i++) {
      CCX_REQUIRE(ctx, shape[i] > 0, "%s: '%s' has an empty dim", model, name);
      n *= (size_t)shape[i];
      t.shape.push_back(shape[i]);
    }
    t.data.resize(n);
    if (dtype == CCX_DTYPE_F32) {
      CCX_HIP(ctx, hipMemcpy(t.data.data(), data, n * 4, hipMemcpyDefault));
    } else if (dtype == CCX_DTYPE_BF16 || dtype == CCX_DTYPE_F16) {
      std::vector<uint16_t> tmp(n);
      CCX_HIP(ctx, hipMemcpy(tmp.data(), data, n * 2, hipMemcpyDefault));
      for (size_t i = 0; i < n; i++) {
        if (dtype == CCX_DTYPE_BF16) { uint32_t u = (uint32_t)tmp[i] << 16; memcpy(&t.data[i], &u, 4); }
        else t.data[i] = ccx_host_half_to_f32(tmp[i]);
      }
    } else {
      return ccx_fail(ctx, CCX_ERR_ARG, "%s: set_tensor dtype %d unsupported", model, dtype);
    }
    staged[std::string(name)] = std::move(t);
    return CCX_OK;
  }
  // f32 by element count: the tensor carries no shape and need() checks its size only
  int stage(const char* name, const float* data, int64_t numel) {
    ccx_host_tensor t;
    t.data.resize((size_t)numel);
    CCX_HIP(ctx, hipMemcpy(t.data.data(), data, (size_t)numel * 4, hipMemcpyDefault));
    staged[std::string(name)] = std::move(t);
    return CCX_OK;
  }

  // ---- lookup (finalize) ----
  // A tensor staged with a shape must have exactly `shape`; one staged by element count must have prod(shape) elements.
  int need(const std::string& name, const std::vector<int64_t>& shape, const ccx_host_tensor** out) {
    auto it = staged.find(name);
    if (it == staged.end()) return ccx_fail(ctx, CCX_ERR_MISSING, "%s: tensor '%s' was never set", model, name.c_str());
    const ccx_host_tensor& t = it->second;
    if (t.shape.empty()) {
      size_t want = 1;
      for (auto v : shape) want *= (size_t)v;
      if (t.data.size() != want)
        return ccx_fail(ctx, CCX_ERR_ARG, "%s: tensor '%s' has %zu elements, expected %zu", model, name.c_str(), t.data.size(), want);
    } else if (t.shape != shape) {
      std::string got, want;
      for (auto v : t.shape) got += std::to_string(v) + ",";
      for (auto v : shape) want += std::to_string(v) + ",";
      return ccx_fail(ctx, CCX_ERR_ARG, "%s: tensor '%s' has shape [%s] expected [%s]", model, name.c_str(), got.c_str(), want.c_str());
    }
    *out = &t;
    return CCX_OK;
  }

  // ---- device memory ----
  // One hipMalloc of the staged tensors' f32 size + `headroom`, rounded up to 2 MB.
  int open_arena(size_t headroom) {
    size_t bytes = 0;
    for (auto& kv : staged) bytes += kv.second.data.size() * 4;
    arena_cap = ccx_align(bytes + headroom, (size_t)2 << 20);
    void* base = nullptr;
    CCX_HIP(ctx, hipMalloc(&base, arena_cap));
    allocs.push_back(base);
    arena = (char*)base;
    arena_off = 0;
    return CCX_OK;
  }
  // `count` elements, 256-byte aligned: from the arena while it fits, a hipMalloc of its own otherwise.
  template <typename T>
  int alloc(T** out, size_t count, bool zero) {
    const size_t bytes = ccx_align(count * sizeof(T), 256);
    void* p = nullptr;
    if (arena && arena_off + bytes <= arena_cap) {
      p = arena + arena_off;
      arena_off += bytes;
    } else {
      CCX_HIP(ctx, hipMalloc(&p, bytes));
      allocs.push_back(p);
    }
    if (zero) CCX_HIP(ctx, hipMemset(p, 0, bytes));
    *out = (T*)p;
    return CCX_OK;
  }
  template <typename T>
  int upload(T** out, const T* src, size_t n) {
    CCX_TRY(alloc(out, n, zero_uploads));
    CCX_HIP(ctx, hipMemcpy(*out, src, n * sizeof(T), hipMemcpyHostToDevice));
    return CCX_OK;
  }
  template <typename T>
  int upload(T** out, const std::vector<T>& src) { return upload(out, src.data(), src.size()); }
  // f32 -> bf16 (round to nearest even) on the host, then upload
  int upload_bf16(bf16_t** out, const float* src, size_t n) {
    std::vector<bf16_t> tmp(n);
    for (size_t i = 0; i < n; i++) tmp[i] = ccx_host_f32_to_bf16(src[i]);
    return upload(out, tmp);
  }
  int upload_bf16(bf16_t** out, const std::vector<float>& src) { return upload_bf16(out, src.data(), src.size()); }

  void free_all() {
    for (void* p : allocs) hipFree(p);
    allocs.clear();
    arena = nullptr;
    arena_cap = arena_off = 0;
  }
};

// `const ccx_host_tensor* var` = the staged tensor `name` of the given shape (or element count), or return the error
#define CCX_NEED(store, var, name, ...)                                             \
  const ccx_host_tensor* var = nullptr;                                             \
  CCX_TRY((store).need((name), std::vector<int64_t>{__VA_ARGS__}, &var))
