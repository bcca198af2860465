// What every host harness under tests/host/ shares.  A harness program is ONE
// translation unit of tests/host/ plus the product source it checks, built with
// -fsanitize=address,undefined on the CPU: include this header once per program.  It
// defines the product's error sink (ga_set_error), CHECK and its failure counter, the
// text log the recording fakes append to, the suite runner, and fakes of the HIP runtime
// calls the host code under test makes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/garage_amd.h"

// ---- the product's error text -------------------------------------------------------
static std::string g_error;  // what the last ga_set_error call said
void ga_set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}

// ---- checks ---------------------------------------------------------------------------
static int g_failed = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++g_failed;                                                         \
    }                                                                     \
  } while (0)

// the end of a program with one suite: the failure count, or the success line
static int finish(const char* ok_line) {
  if (g_failed) {
    fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("%s\n", ok_line);
  return 0;
}

// A program with several suites runs those named on its command line, in that order,
// or all of them.  A suite sets every switch it depends on itself, so any order passes;
// each prints its success line when none of its checks failed.
struct Suite {
  const char* name;
  void (*run)();
  const char* ok_line;
};
static int run_suites(const std::vector<Suite>& suites, int argc, char** argv) {
  std::vector<const Suite*> chosen;
  for (int i = 1; i < argc; ++i) {
    const Suite* found = nullptr;
    for (const Suite& s : suites)
      if (!strcmp(s.name, argv[i])) found = &s;
    if (!found) {
      fprintf(stderr, "no suite '%s'\n", argv[i]);
      return 2;
    }
    chosen.push_back(found);
  }
  if (chosen.empty())
    for (const Suite& s : suites) chosen.push_back(&s);
  for (const Suite* s : chosen) {
    const int before = g_failed;
    s->run();
    if (g_failed == before)
      printf("%s\n", s->ok_line);
    else
      fprintf(stderr, "%s: %d check(s) failed\n", s->name, g_failed - before);
  }
  return g_failed ? 1 : 0;
}

// ---- the text log -------------------------------------------------------------------
static std::vector<std::string> g_log;
static void logf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_log.push_back(buf);
}
// lines that begin with `prefix`
static int count(const char* prefix) {
  int n = 0;
  for (auto& l : g_log) n += l.rfind(prefix, 0) == 0;
  return n;
}
// ... and the M= that follows the prefix in each of them
static std::vector<long long> ms_of(const char* prefix) {
  std::vector<long long> out;
  for (auto& l : g_log)
    if (l.rfind(prefix, 0) == 0) {
      long long m = -1;
      sscanf(l.c_str() + strlen(prefix), " M=%lld", &m);
      out.push_back(m);
    }
  return out;
}

// ---- HIP runtime fakes ----------------------------------------------------------------
// "Device" memory is host memory of exactly the size asked for, a copy happens at once,
// an event is a slot of a static ring.  Waits, records and memsets go to the text log;
// the allocations, copies and records are counted as well.
static std::vector<size_t> g_host_allocs, g_dev_allocs, g_copies;  // bytes of each call
static int g_events_recorded = 0;
static int g_device = 0;  // what hipGetDevice answers
static bool g_hip_malloc_fails = false;  // hipMalloc answers hipErrorOutOfMemory

extern "C" {
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
  g_host_allocs.push_back(bytes);
  *p = malloc(bytes);
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) {
  if (g_hip_malloc_fails) return hipErrorOutOfMemory;
  g_dev_allocs.push_back(bytes);
  *p = malloc(bytes);
  return hipSuccess;
}
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind,
                          hipStream_t) {
  g_copies.push_back(bytes);
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void*, int, size_t bytes, hipStream_t) {
  logf("memset %zu", bytes);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  static char slots[64];
  static int next = 0;
  *e = (hipEvent_t)&slots[next++ % 64];
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  logf("record stream=%p event=%p", (void*)s, (void*)e);
  ++g_events_recorded;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  logf("wait stream=%p event=%p", (void*)s, (void*)e);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = g_device; return hipSuccess; }
}  // extern "C"

// ---- the one kernel-side answer two fake sides share ------------------------------------
// (rollout_loop.cpp and mlp_layers.cpp both ask it; a program that links the real one,
// rollout_host.cpp's, defines GA_HARNESS_REAL_STEP_PREDICATE before it includes this)
#ifndef GA_HARNESS_REAL_STEP_PREDICATE
static int g_policy_step_fused_ok = 1;
extern "C" int ga_policy_step_fused_supported(const ga_mlp_desc* d) {
  return g_policy_step_fused_ok && d->n_layers >= 1;
}
#endif
