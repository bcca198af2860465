// Tables a host entry point builds per call and its launches read from the device: pinned
// host memory and its device copy, a ring of them.  A call's launches read the device copy
// after the call has returned, and the copy reads the pinned memory, so a call takes the
// next of RING slots and `done` (recorded behind the call's last launch) is waited for
// before the slot is rewritten -- RING calls later: the one place where such an entry point
// may block its caller.  Written once for ga_update_epoch_members (update_members.cpp) and
// the population entries of the linear feature baseline (linear_baseline_members_host.cpp);
// each of them owns one ring and its mutex.  Host C++ only: the HIP runtime calls are the
// ones tests/host/harness.h fakes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <mutex>

struct GaTableSlot {
  void* host = nullptr;
  void* dev = nullptr;
  size_t capacity = 0;  // bytes of each; grows, never shrinks
  int device = -1;      // the device `dev` lives on
  hipEvent_t done = nullptr;
  bool pending = false;
};

struct GaTableRing {
  static constexpr int RING = 8;
  GaTableSlot slots[RING];
  int next = 0;
  std::mutex mu;  // held by the entry point from take() to mark_done()

  static void slot_free(GaTableSlot& s) {
    if (s.host) (void)hipHostFree(s.host);
    if (s.dev) (void)hipFree(s.dev);
    s.host = s.dev = nullptr;
    s.capacity = 0;
    s.device = -1;
  }

  // The next slot, idle and holding at least `bytes` on the current device.  A slot is
  // re-allocated only to grow (to exactly `bytes`) or when the current device is another:
  // calls whose sizes differ a little from one to the next reuse it as it is.
  GaTableSlot* take(size_t bytes) {
    GaTableSlot& s = slots[next];
    next = (next + 1) % RING;
    if (s.pending) {
      if (hipEventSynchronize(s.done) != hipSuccess) return nullptr;
      s.pending = false;
    }
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return nullptr;
    if (s.device != device && s.done) {  // (an event belongs to its device too)
      (void)hipEventDestroy(s.done);
      s.done = nullptr;
    }
    if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) {
      s.done = nullptr;
      return nullptr;
    }
    if (s.capacity < bytes || s.device != device) {
      slot_free(s);
      if (hipHostMalloc(&s.host, bytes, hipHostMallocDefault) != hipSuccess) {
        s.host = nullptr;
        return nullptr;
      }
      if (hipMalloc(&s.dev, bytes) != hipSuccess) {
        s.dev = nullptr;
        slot_free(s);
        return nullptr;
      }
      s.capacity = bytes;
      s.device = device;
    }
    return &s;
  }

  // The first `bytes` of the slot's pinned memory to its device copy, on `stream`.  From
  // this copy on the stream may read the slot: whatever happens after it, the caller ends
  // with mark_done and the slot counts as in flight until then.
  static bool upload(GaTableSlot* s, size_t bytes, hipStream_t stream) {
    s->pending = true;
    return hipMemcpyAsync(s->dev, s->host, bytes, hipMemcpyHostToDevice, stream) ==
           hipSuccess;
  }

  // The event behind what was enqueued.  false: it could not be recorded -- nothing marks
  // the end of what reads the slot, so the stream was waited for here instead.
  static bool mark_done(GaTableSlot* s, hipStream_t stream) {
    if (hipEventRecord(s->done, stream) == hipSuccess) return true;
    (void)hipStreamSynchronize(stream);
    s->pending = false;
    return false;
  }

  // frees every slot (tests; the library otherwise keeps them for its lifetime)
  void release() {
    std::lock_guard<std::mutex> lock(mu);
    for (GaTableSlot& s : slots) {
      if (s.pending) (void)hipEventSynchronize(s.done);
      s.pending = false;
      slot_free(s);
    }
  }
};
