// hip_mock_async.h -- TEST ONLY.  hip_mock.h plus the stream-ordered calls of icerx_decode_device_async (decoder_async.hpp):
// the mock has no queues, so an async copy / memset is a plain one and events are names only.  Built by
// tests/test_decoder_async_emu.py (g++ -x c++ -DICER_HOST_MOCK -DICER_WAVE_EMU -include tests/emu/hip_mock_async.h ...).
#pragma once
#include "hip_mock.h"

#define ICER_MOCK_ASYNC 1
typedef void *hipEvent_t;
static const unsigned hipEventDisableTiming = 2;
static inline hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
static inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { static char name; *e = &name; return hipSuccess; }
static inline hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
