// The owners of the context's HIP handles (3dobjecttracking_amd/csrc/m3t_host_resources.h) on the host, with stand-ins
// in the place of the runtime functions the header calls: they count what is live, note the flags they were given and
// fail the k-th call of a function on request.  Every case ends with nothing live.  Prints "checks N errors M".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../../3dobjecttracking_amd/csrc/m3t_host_resources.h"

using namespace m3t_res;

static int g_checks = 0, g_errors = 0;
#define CHECK(cond)                                  \
  do {                                               \
    ++g_checks;                                      \
    if (!(cond)) {                                   \
      ++g_errors;                                    \
      std::printf("line %d: %s\n", __LINE__, #cond); \
    }                                                \
  } while (0)

// ---- the stand-ins -----------------------------------------------------------------------------------------------
enum Call { kEventCreate, kStreamCreate, kMaskedStreamCreate, kHostMalloc, kDevicePointer, kMalloc, kCalls };
static int g_fail_at[kCalls];  // the call of that function that fails, counting down from here (0: none)
static int g_calls[kCalls];
static std::set<void*> g_events, g_streams, g_host, g_device;
static int g_double_destroys = 0;
static unsigned g_last_flags = 0, g_host_flags = 0;  // of the last event / stream, of the last host block
static std::vector<void*> g_waited, g_recorded, g_host_freed;

static bool Fails(Call c) {
  ++g_calls[c];
  return g_fail_at[c] > 0 && --g_fail_at[c] == 0;
}
static void* NewHandle(std::set<void*>* live, size_t bytes = 1) {
  void* p = std::malloc(bytes);
  std::memset(p, 0xab, bytes);
  live->insert(p);
  return p;
}
static hipError_t Drop(std::set<void*>* live, void* p) {
  if (!live->erase(p)) {
    ++g_double_destroys;
    return hipErrorInvalidValue;
  }
  std::free(p);
  return hipSuccess;
}
static bool NothingLive() {
  return g_events.empty() && g_streams.empty() && g_host.empty() && g_device.empty() && g_double_destroys == 0;
}

extern "C" {
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags) {
  if (Fails(kEventCreate)) return hipErrorOutOfMemory;
  g_last_flags = flags;
  *event = static_cast<hipEvent_t>(NewHandle(&g_events));
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) { return Drop(&g_events, event); }
hipError_t hipEventSynchronize(hipEvent_t event) {
  g_waited.push_back(event);
  return g_events.count(event) ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t) {
  g_recorded.push_back(event);
  return g_events.count(event) ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned flags) {
  if (Fails(kStreamCreate)) return hipErrorOutOfMemory;
  g_last_flags = flags;
  *stream = static_cast<hipStream_t>(NewHandle(&g_streams));
  return hipSuccess;
}
hipError_t hipExtStreamCreateWithCUMask(hipStream_t* stream, uint32_t words, const uint32_t* mask) {
  if (Fails(kMaskedStreamCreate)) return hipErrorOutOfMemory;
  g_last_flags = 0;
  for (uint32_t i = 0; i < words; ++i) g_last_flags += unsigned(__builtin_popcount(mask[i]));  // (the CUs of the mask)
  *stream = static_cast<hipStream_t>(NewHandle(&g_streams));
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) { return Drop(&g_streams, stream); }
hipError_t hipHostMalloc(void** ptr, size_t bytes, unsigned flags) {
  if (Fails(kHostMalloc)) return hipErrorOutOfMemory;
  g_host_flags = flags;
  *ptr = NewHandle(&g_host, bytes);
  return hipSuccess;
}
hipError_t hipHostFree(void* ptr) {
  g_host_freed.push_back(ptr);
  return Drop(&g_host, ptr);
}
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) {
  if (Fails(kDevicePointer)) return hipErrorInvalidValue;
  *dev = static_cast<char*>(host) + 1;  // (never dereferenced)
  return hipSuccess;
}
hipError_t hipMalloc(void** ptr, size_t bytes) {
  if (Fails(kMalloc)) return hipErrorOutOfMemory;
  *ptr = NewHandle(&g_device, bytes);
  return hipSuccess;
}
hipError_t hipFree(void* ptr) { return Drop(&g_device, ptr); }
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
}

// ---- the cases ---------------------------------------------------------------------------------------------------
static void Events() {
  {
    Event e;
    CHECK(!e && e.get() == nullptr && g_calls[kEventCreate] == 0);  // nothing before the first use
    CHECK(e.Ensure(hipEventDisableTiming) == hipSuccess && g_last_flags == hipEventDisableTiming);
    const hipEvent_t first = e.get();
    CHECK(e.Ensure(hipEventDisableTiming) == hipSuccess && e.get() == first && g_calls[kEventCreate] == 1);
    CHECK(g_events.size() == 1);
    Event moved(std::move(e));
    CHECK(moved.get() == first && !e && g_events.size() == 1);
    Event other;
    CHECK(other.Ensure(hipEventDefault) == hipSuccess && g_last_flags == hipEventDefault && g_events.size() == 2);
    other = std::move(moved);  // the event `other` held goes, exactly once
    CHECK(other.get() == first && !moved && g_events.size() == 1);
  }
  CHECK(NothingLive());
  {
    std::vector<Event> v(2);
    for (Event& e : v) CHECK(e.Ensure(hipEventDisableTiming) == hipSuccess);
    const hipEvent_t first = v[0].get();
    v.resize(9);  // (reallocates: the handles move)
    CHECK(v[0].get() == first && !v[8] && g_events.size() == 2);
    CHECK(v[8].Ensure(hipEventDisableTiming) == hipSuccess && g_events.size() == 3);
    v.resize(1);
    CHECK(v[0].get() == first && g_events.size() == 1);
  }
  CHECK(NothingLive());
}

static void Streams() {
  {
    Stream a, b;
    CHECK(CreateMaskedStream(0, 256, &a, false) == hipSuccess && g_last_flags == hipStreamNonBlocking);
    CHECK(CreateMaskedStream(32, 256, &b, true) == hipSuccess && g_last_flags == 32);    // the ingest side: 32 CUs
    const hipStream_t old = a.get(), made = b.get();
    a = std::move(b);
    CHECK(a.get() == made && !b && g_streams.size() == 1 && !g_streams.count(old));
    CHECK(CreateMaskedStream(32, 256, &b, false) == hipSuccess && g_last_flags == 224);  // the compute side: the rest
  }
  CHECK(NothingLive());
}

static void HostBlocks() {
  {
    HostBlock b;
    CHECK(b.Alloc(64, hipHostMallocMapped, true) == hipSuccess && g_host_flags == hipHostMallocMapped);
    CHECK(b.host && b.dev && b.bytes == 64);
    bool zero = true;
    for (size_t i = 0; i < 64; ++i) zero = zero && b.as<unsigned char>()[i] == 0;
    CHECK(zero);
    void* old = b.host;
    g_host_freed.clear();
    CHECK(b.Alloc(128, hipHostMallocDefault, false) == hipSuccess && g_host_flags == hipHostMallocDefault);
    CHECK(g_host_freed.size() == 1 && g_host_freed[0] == old && g_host.size() == 1);  // the old block went first
    CHECK(b.host && !b.dev && b.bytes == 128 && b.as<unsigned char>()[0] == 0xab);   // pinned only, not zeroed
    g_fail_at[kHostMalloc] = 1;
    CHECK(b.Alloc(256, hipHostMallocMapped, true) == hipErrorOutOfMemory);
    CHECK(!b.host && !b.dev && b.bytes == 0 && g_host.empty());
    CHECK(b.Alloc(256, hipHostMallocMapped, true) == hipSuccess && g_host.size() == 1);
    g_fail_at[kDevicePointer] = 1;
    CHECK(b.Alloc(512, hipHostMallocMapped, true) == hipErrorInvalidValue);
    CHECK(!b.host && !b.dev && b.bytes == 0 && g_host.empty());
    CHECK(b.Alloc(32, hipHostMallocMapped, false) == hipSuccess);
    HostBlock moved(std::move(b));
    CHECK(moved.bytes == 32 && !b.host && b.bytes == 0 && g_host.size() == 1);
  }
  CHECK(NothingLive());
  {
    DevMem table;
    const std::vector<int> none, three = {1, 2, 3};
    CHECK(UploadTable(&table, none) == hipSuccess && table.bytes == sizeof(int));  // room for one element
    CHECK(UploadTable(&table, three) == hipSuccess && table.bytes == 3 * sizeof(int) && table.as<int>()[2] == 3);
    CHECK(g_device.size() == 1);
    g_fail_at[kMalloc] = 1;
    CHECK(UploadTable(&table, three) == hipErrorOutOfMemory && !table.p && table.bytes == 0);
  }
  CHECK(NothingLive());
}

// the enqueued calls' ring: mapped blocks, each grown on its own
static void MappedRing() {
  {
    HostRing<4, hipHostMallocMapped> ring;
    hipEvent_t done[4] = {nullptr, nullptr, nullptr, nullptr};
    void* block[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int turn = 0; turn < 6; ++turn) {
      void *host = nullptr, *dev = nullptr;
      int slot = -1;
      g_waited.clear();
      g_recorded.clear();
      CHECK(ring.Acquire(100, &host, &dev, &slot) == hipSuccess && slot == turn % 4 && host && dev && g_host_flags == hipHostMallocMapped);
      CHECK(g_waited.size() == 1 && g_waited[0] == ring.done[slot].get());
      if (turn < 4) {
        done[slot] = ring.done[slot].get();
        block[slot] = host;
        CHECK(g_events.size() == size_t(turn + 1) && g_host.size() == size_t(turn + 1));  // made as they are first taken
      } else {
        CHECK(g_waited[0] == done[slot] && host == block[slot]);  // the slot of four turns ago, and its event
      }
      CHECK(ring.block[slot].bytes == 200);
      CHECK(ring.Release(slot, nullptr) == hipSuccess && g_recorded.size() == 1 && g_recorded[0] == done[slot]);
    }
    CHECK(g_events.size() == 4 && g_host.size() == 4);
    void *host = nullptr, *dev = nullptr;
    int slot = -1;
    g_host_freed.clear();
    CHECK(ring.Acquire(201, &host, &dev, &slot) == hipSuccess && slot == 2);  // a larger request: that slot alone grows
    CHECK(g_host_freed.size() == 1 && g_host_freed[0] == block[2] && host != nullptr);
    CHECK(ring.block[2].bytes == 402 && ring.block[0].bytes == 200 && ring.block[1].bytes == 200 && ring.block[3].bytes == 200);
    CHECK(ring.Release(slot, nullptr) == hipSuccess);
  }
  CHECK(NothingLive());
  {
    HostRing<4, hipHostMallocMapped> ring;
    void *host = nullptr, *dev = nullptr;
    int slot = -1;
    for (int turn = 0; turn < 2; ++turn) {
      CHECK(ring.Acquire(64, &host, &dev, &slot) == hipSuccess);
      CHECK(ring.Release(slot, nullptr) == hipSuccess);
    }
    g_fail_at[kHostMalloc] = 1;
    CHECK(ring.Acquire(64, &host, &dev, &slot) == hipErrorOutOfMemory && slot == 2);  // turn 3
    CHECK(!ring.block[2].host && ring.block[2].bytes == 0 && g_host.size() == 2);
    CHECK(ring.Acquire(64, &host, &dev, &slot) == hipSuccess && slot == 3 && host);     // turn 4
    CHECK(ring.Release(slot, nullptr) == hipSuccess);
    for (int turn = 4; turn < 7; ++turn) {  // ... and slot 2 is allocated when its turn comes again
      CHECK(ring.Acquire(64, &host, &dev, &slot) == hipSuccess && slot == turn % 4 && host == ring.block[slot].host);
      CHECK(ring.Release(slot, nullptr) == hipSuccess);
    }
    CHECK(ring.block[2].bytes == 128 && g_host.size() == 4);
  }
  CHECK(NothingLive());
}

// the camera table's staging ring: pinned blocks, all of them grown at once (the user has synchronised its stream)
static void StagingRing() {
  {
    HostRing<8, hipHostMallocDefault> ring;
    CHECK(ring.SmallestBlock() == 0);
    CHECK(ring.GrowAll(100) == hipSuccess && g_host_flags == hipHostMallocDefault);
    CHECK(g_host.size() == 8 && g_events.size() == 8 && ring.SmallestBlock() == 200);
    const int allocations = g_calls[kHostMalloc];
    for (int turn = 0; turn < 10; ++turn) {  // more turns than blocks
      void* host = nullptr;
      int slot = -1;
      g_waited.clear();
      CHECK(ring.Acquire(100, &host, nullptr, &slot) == hipSuccess && slot == turn % 8 && host == ring.block[slot].host);
      CHECK(g_waited.size() == 1 && g_waited[0] == ring.done[slot].get());
      CHECK(ring.Release(slot, nullptr) == hipSuccess);
    }
    CHECK(g_calls[kHostMalloc] == allocations && g_events.size() == 8);
    g_host_freed.clear();
    CHECK(ring.SmallestBlock() < 201 && ring.GrowAll(201) == hipSuccess);  // growth: all eight
    CHECK(g_host_freed.size() == 8 && g_host.size() == 8 && g_events.size() == 8);
    for (const HostBlock& b : ring.block) CHECK(b.bytes == 402 && b.host && !b.dev);
    // block 5 of 8 fails: what is left says so, and the next request of the same size asks again
    g_fail_at[kHostMalloc] = 5;
    CHECK(ring.GrowAll(1000) == hipErrorOutOfMemory);
    for (int i = 0; i < 8; ++i) {
      const HostBlock& b = ring.block[i];
      CHECK(b.bytes == (i < 4 ? 2000u : i == 4 ? 0u : 402u) && (b.host != nullptr) == (i != 4) && g_host.count(b.host) == (i != 4));
    }
    CHECK(ring.SmallestBlock() == 0 && g_host.size() == 7);
    CHECK(ring.GrowAll(1000) == hipSuccess && ring.SmallestBlock() == 2000 && g_host.size() == 8);
    void* host = nullptr;
    int slot = -1;
    CHECK(ring.Acquire(1000, &host, nullptr, &slot) == hipSuccess && host == ring.block[slot].host && g_host.count(host));
    CHECK(ring.Release(slot, nullptr) == hipSuccess);
  }
  CHECK(NothingLive());
}

static void TimerPair() {
  {
    EventPair pair;
    g_fail_at[kEventCreate] = 2;
    CHECK(pair.Ensure(hipEventDefault) == hipErrorOutOfMemory);
    CHECK(!pair && !pair.a && !pair.b && g_events.empty());  // the first event went with the failure of the second
    CHECK(pair.Ensure(hipEventDefault) == hipSuccess && g_last_flags == hipEventDefault && g_events.size() == 2);
    struct Pending {
      EventPair events;
      int which;
    };
    std::vector<Pending> pending;
    pending.push_back({std::move(pair), 1});
    CHECK(!pair && g_events.size() == 2);
    for (int i = 0; i < 5; ++i) {
      EventPair more;
      CHECK(more.Ensure(hipEventDefault) == hipSuccess);
      pending.push_back({std::move(more), 0});
    }
    CHECK(g_events.size() == 12);
  }  // a context destroyed with pairs pending
  CHECK(NothingLive());
}

// m3t_hip_reserve_ingest_cus: all new streams first, then the swap
static void IngestCuSequence() {
  constexpr int kCopyStreams = 4;
  {
    Stream compute, copy[kCopyStreams];
    CHECK(CreateMaskedStream(0, 256, &compute, false) == hipSuccess);
    for (Stream& s : copy) CHECK(s.Create(hipStreamNonBlocking) == hipSuccess);
    const std::set<void*> old = g_streams;
    auto make = [&](Stream* new_compute, Stream (&new_copy)[kCopyStreams]) {
      hipError_t e = CreateMaskedStream(32, 256, new_compute, false);
      if (e == hipSuccess) e = CreateMaskedStream(32, 256, &new_copy[0], true);
      for (int i = 1; i < kCopyStreams && e == hipSuccess; ++i) e = new_copy[i].Create(hipStreamNonBlocking);
      return e;
    };
    {
      Stream new_compute, new_copy[kCopyStreams];
      g_fail_at[kStreamCreate] = 1;  // the third creation: two masked streams, then the first plain one
      g_calls[kStreamCreate] = g_calls[kMaskedStreamCreate] = 0;
      CHECK(make(&new_compute, new_copy) == hipErrorOutOfMemory);
      CHECK(g_calls[kMaskedStreamCreate] == 2 && g_calls[kStreamCreate] == 1 && g_streams.size() == old.size() + 2);
    }
    CHECK(g_streams == old);  // the old streams untouched, no new stream live
    {
      Stream new_compute, new_copy[kCopyStreams];
      CHECK(make(&new_compute, new_copy) == hipSuccess);
      compute = std::move(new_compute);
      for (int i = 0; i < kCopyStreams; ++i) copy[i] = std::move(new_copy[i]);
    }
    CHECK(g_streams.size() == old.size());
    for (void* s : old) CHECK(!g_streams.count(s));
  }
  CHECK(NothingLive());
}

int main() {
  Events();
  Streams();
  HostBlocks();
  MappedRing();
  StagingRing();
  TimerPair();
  IngestCuSequence();
  std::printf("checks %d errors %d\n", g_checks, g_errors);
  return g_errors ? 1 : 0;
}
