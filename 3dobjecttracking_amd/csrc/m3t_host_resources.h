// m3t_host_resources.h — the owners of every HIP handle of a context: device memory, events, streams, pinned and mapped
// host memory, and the ring of host blocks the enqueued calls and the camera table take in turn.  The only place in
// csrc/ that creates or destroys one of these; a new handle becomes a member of one of these types.  Host code alone
// (runtime API and the standard library): tests/cpp/host_resources_check.cpp runs it against stand-ins for the runtime.
#pragma once

#if !defined(__HIP_PLATFORM_AMD__) && !defined(__HIP_PLATFORM_NVIDIA__)
#define __HIP_PLATFORM_AMD__ 1  // a host compiler, without hipcc's own definition
#endif
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace m3t_res {

struct DevMem {
  void* p = nullptr;
  size_t bytes = 0;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  hipError_t alloc(size_t n) {
    release();
    if (n == 0) n = 16;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

// "This vector is that device table": room for max(1, size) elements, then a blocking copy of what there is.
template <typename T>
hipError_t UploadTable(DevMem* table, const std::vector<T>& v) {
  hipError_t e = table->alloc(std::max<size_t>(1, v.size()) * sizeof(T));
  if (e == hipSuccess && !v.empty()) e = hipMemcpy(table->p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) {
      Reset();
      e_ = o.e_;
      o.e_ = nullptr;
    }
    return *this;
  }
  ~Event() { Reset(); }
  hipError_t Ensure(unsigned flags) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }  // made on first use
  hipEvent_t get() const { return e_; }
  explicit operator bool() const { return e_ != nullptr; }
  void Reset() {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }

 private:
  hipEvent_t e_ = nullptr;
};

// The two events around a timed stretch of launches: both or neither.
struct EventPair {
  Event a, b;
  hipError_t Ensure(unsigned flags) {
    hipError_t e = a.Ensure(flags);
    if (e == hipSuccess) e = b.Ensure(flags);
    if (e != hipSuccess) a.Reset(), b.Reset();
    return e;
  }
  explicit operator bool() const { return bool(a); }
};

class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) {
      Reset();
      s_ = o.s_;
      o.s_ = nullptr;
    }
    return *this;
  }
  ~Stream() { Reset(); }
  hipError_t Create(unsigned flags) {
    Reset();
    return hipStreamCreateWithFlags(&s_, flags);
  }
  hipError_t CreateWithCUMask(const std::vector<uint32_t>& mask) {
    Reset();
    return hipExtStreamCreateWithCUMask(&s_, uint32_t(mask.size()), mask.data());
  }
  hipStream_t get() const { return s_; }
  explicit operator bool() const { return s_ != nullptr; }
  void Reset() {
    if (s_) (void)hipStreamDestroy(s_);
    s_ = nullptr;
  }

 private:
  hipStream_t s_ = nullptr;
};

// A stream of the context.  With CUs reserved for ingest (m3t_hip_reserve_ingest_cus) the compute stream runs on the
// CUs of mask bits [0, CUs - n) and copy stream 0 -- the one the ROI pull kernel is launched on -- on bits
// [CUs - n, CUs).  Bit i of a mask belongs to XCD i mod 8 (amdkfd deals the bits round-robin; tools/ubench_cumask.hip
// counts 30 / 2 CUs per XCD for 240 / 16 bits), inside an XCD the highest bits are the last CU of each shader engine.
inline hipError_t CreateMaskedStream(int ingest_cus, int cus, Stream* stream, bool ingest_side) {
  if (ingest_cus <= 0) return stream->Create(hipStreamNonBlocking);
  const int split = cus - ingest_cus;
  std::vector<uint32_t> mask(size_t(cus + 31) / 32, 0u);
  for (int i = ingest_side ? split : 0; i < (ingest_side ? cus : split); ++i) mask[size_t(i) / 32] |= 1u << (i % 32);
  return stream->CreateWithCUMask(mask);
}

// Pinned host memory; with kMapped among the flags the kernels read and write it in place through `dev`.
constexpr unsigned kPinned = hipHostMallocDefault, kMapped = hipHostMallocMapped;
struct HostBlock {
  void* host = nullptr;
  void* dev = nullptr;
  size_t bytes = 0;
  HostBlock() = default;
  HostBlock(const HostBlock&) = delete;
  HostBlock& operator=(const HostBlock&) = delete;
  HostBlock(HostBlock&& o) noexcept : host(o.host), dev(o.dev), bytes(o.bytes) { o.Forget(); }
  HostBlock& operator=(HostBlock&& o) noexcept {
    if (this != &o) {
      (void)Free();
      host = o.host, dev = o.dev, bytes = o.bytes;
      o.Forget();
    }
    return *this;
  }
  ~HostBlock() { (void)Free(); }
  hipError_t Free() {
    const hipError_t e = host ? hipHostFree(host) : hipSuccess;
    Forget();
    return e;
  }
  // the previous block goes first; any failure leaves the object empty
  hipError_t Alloc(size_t n, unsigned flags, bool zero) {
    hipError_t e = Free();
    if (e != hipSuccess || (e = hipHostMalloc(&host, n, flags)) != hipSuccess) {
      Forget();
      return e;
    }
    bytes = n;
    if (zero) std::memset(host, 0, n);
    if ((flags & kMapped) && (e = hipHostGetDevicePointer(&dev, host, 0)) != hipSuccess) (void)Free();
    return e;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(host); }
  template <typename T>
  T* dev_as() const { return static_cast<T*>(dev); }

 private:
  void Forget() {
    host = dev = nullptr;
    bytes = 0;
  }
};

// kDepth host blocks taken in turn, each guarded by an event recorded behind its last use: a call fills its block, the
// work it enqueues reads it, and the call kDepth calls later waits for that work before it takes the block again.
// Acquire grows the one block it takes, behind that block's event.  GrowAll grows every block, for a user that has
// synchronised the stream the blocks were last used on.
template <int kDepthT, unsigned kFlags>
struct HostRing {
  static constexpr int kDepth = kDepthT;
  HostBlock block[kDepth];
  Event done[kDepth];
  int next = 0;
  size_t SmallestBlock() const {
    size_t n = block[0].bytes;
    for (const HostBlock& b : block) n = std::min(n, b.bytes);
    return n;
  }
  hipError_t GrowAll(size_t n) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < kDepth && e == hipSuccess; ++i)
      if ((e = Grow(i, n)) == hipSuccess) e = done[i].Ensure(hipEventDisableTiming);
    return e;
  }
  hipError_t Acquire(size_t n, void** host, void** dev, int* slot) {
    const int s = *slot = next;
    next = (s + 1) % kDepth;
    hipError_t e = done[s].Ensure(hipEventDisableTiming);
    if (e != hipSuccess) return e;
    if ((e = hipEventSynchronize(done[s].get())) != hipSuccess) return e;  // the call kDepth calls ago: normally long complete
    if ((e = Grow(s, n)) != hipSuccess) return e;
    *host = block[s].host;
    if (dev) *dev = block[s].dev;
    return hipSuccess;
  }
  hipError_t Release(int slot, hipStream_t stream) { return hipEventRecord(done[slot].get(), stream); }

 private:
  hipError_t Grow(int s, size_t n) { return block[s].bytes >= n ? hipSuccess : block[s].Alloc(n * 2, kFlags, false); }
};

}  // namespace m3t_res
