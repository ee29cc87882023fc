// op_scratch.h -- what the stand-alone operator entry points (dec_ops.hip, sep_ops.hip, align.hip) share: device scratch of one call
// and the alignment test of their descriptors' pointers.
#pragma once
#include <stdint.h>
#include <vector>
#include <hip/hip_runtime.h>

// device scratch of one call: everything allocated through it is freed when it goes out of scope
struct ccx_op_scratch {
  std::vector<void*> ptrs;
  ~ccx_op_scratch() { for (void* p : ptrs) hipFree(p); }
  template <class T>
  hipError_t alloc(T** out, size_t n) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, (n ? n : 1) * sizeof(T));
    if (e == hipSuccess) { ptrs.push_back(p); *out = (T*)p; }
    return e;
  }
  template <class T>
  hipError_t upload(T** out, const T* src, size_t n) {
    hipError_t e = alloc(out, n);
    if (e == hipSuccess) e = hipMemcpy(*out, src, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
};

static inline bool ccx_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
