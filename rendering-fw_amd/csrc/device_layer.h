// device_layer.h — namespace dm: device memory, copies, streams and events of the host layer (rfwhip_api.cpp, rfwhip_group.cpp).
//
// Three back ends behind one set of signatures, selected as everywhere else:
//   (no RFWHIP_HOST_EMULATION)   HIP: the product
//   RFWHIP_EMU_STREAMS           the emulation's heap with deferred streams: emu_streams.h schedules every operation
//   otherwise                    the emulation's heap, "streams" are immediate
// Every HIP runtime call of the host layer stands here and nowhere else.  Failures go through rfwhip_internal_set_error,
// so both translation units share the thread's rfwhip_last_error() text.  A stream is a void * (hipStream_t in the product).
#pragma once
#include "rfwhip.h"

#include "internal.h"

#include <chrono>
#include <stdlib.h>
#include <string.h>

#if !defined(RFWHIP_HOST_EMULATION)
#include <hip/hip_runtime.h>
#endif
#include "emu_streams.h" // (the deferred-stream variant of the emulation build; empty otherwise)

namespace dm
{
#if !defined(RFWHIP_HOST_EMULATION)
#define DM_CHECK(x)                                                                                                  \
	do                                                                                                               \
	{                                                                                                                \
		const hipError_t e_ = (x);                                                                                   \
		if (e_ != hipSuccess)                                                                                        \
			return rfwhip_internal_set_error(RFWHIP_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
	} while (0)

inline int device_count()
{
	int n = 0;
	return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
inline int init(int device, int *cus)
{
	const int n = device_count();
	if (n <= 0)
		return rfwhip_internal_set_error(RFWHIP_ERR_NO_DEVICE, "no HIP device visible: the rendercore has no CPU path");
	if (device < 0 || device >= n)
		return rfwhip_internal_set_error(RFWHIP_ERR_NO_DEVICE, "device ordinal %d out of range (%d devices)", device, n);
	DM_CHECK(hipSetDevice(device));
	hipDeviceProp_t prop;
	DM_CHECK(hipGetDeviceProperties(&prop, device));
	*cus = prop.multiProcessorCount;
	return 0;
}
inline int use(int device)
{
	DM_CHECK(hipSetDevice(device));
	return 0;
}
inline void enable_peer(int a, int b) // best effort: without it hipMemcpyPeerAsync stages through the host
{
	int can = 0;
	if (a == b || hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can)
		return;
	if (hipSetDevice(a) == hipSuccess)
		(void)hipDeviceEnablePeerAccess(b, 0); // (hipErrorPeerAccessAlreadyEnabled is fine)
	(void)hipGetLastError();
}
inline int alloc(void **p, size_t bytes)
{
	DM_CHECK(hipMalloc(p, bytes ? bytes : 16));
	return 0;
}
inline void release(void *p)
{
	if (p)
		(void)hipFree(p);
}
inline int host_alloc(void **p, size_t bytes) // pinned: a device-to-host copy into it runs asynchronously
{
	DM_CHECK(hipHostMalloc(p, bytes ? bytes : 16, hipHostMallocDefault));
	return 0;
}
inline void host_free(void *p)
{
	if (p)
		(void)hipHostFree(p);
}
inline void mem_info(size_t *free_b, size_t *total_b)
{
	if (hipMemGetInfo(free_b, total_b) != hipSuccess)
		*free_b = *total_b = ~(size_t)0;
}
inline int h2d(void *d, const void *h, size_t n, void *s)
{
	if (n)
		DM_CHECK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, (hipStream_t)s));
	return 0;
}
inline int d2h_async(void *h, const void *d, size_t n, void *s)
{
	if (n)
		DM_CHECK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, (hipStream_t)s));
	return 0;
}
inline int d2d(void *dst, const void *src, size_t n, void *s)
{
	if (n)
		DM_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)s));
	return 0;
}
// dst on dst_device <- src on src_device, enqueued on `s` (a stream of the source device: the copy is pushed)
inline int copy_async(void *dst, int dst_device, const void *src, int src_device, size_t n, void *s)
{
	if (dst_device == src_device)
		return d2d(dst, src, n, s);
	DM_CHECK(hipMemcpyPeerAsync(dst, dst_device, src, src_device, n, (hipStream_t)s));
	return 0;
}
inline int zero(void *d, size_t n, void *s)
{
	if (n)
		DM_CHECK(hipMemsetAsync(d, 0, n, (hipStream_t)s));
	return 0;
}
inline int sync(void *s)
{
	DM_CHECK(hipStreamSynchronize((hipStream_t)s));
	return 0;
}
inline int stream_create(void **s)
{
	hipStream_t st;
	DM_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
	*s = st;
	return 0;
}
inline void stream_destroy(void *s)
{
	if (s)
		(void)hipStreamDestroy((hipStream_t)s);
}
inline int last_launch_error()
{
	DM_CHECK(hipGetLastError());
	return 0;
}
typedef hipEvent_t event_t;
inline int event_create(event_t *e, bool timed = true) // (timed: event_ms may read it; the group's ordering events are not)
{
	if (timed)
		DM_CHECK(hipEventCreate(e));
	else
		DM_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
	return 0;
}
inline void event_destroy(event_t e) { (void)hipEventDestroy(e); }
inline int event_record(event_t &e, void *s)
{
	DM_CHECK(hipEventRecord(e, (hipStream_t)s));
	return 0;
}
inline float event_ms(event_t a, event_t b)
{
	float ms = 0;
	if (hipEventElapsedTime(&ms, a, b) != hipSuccess)
		return 0.0f;
	return ms;
}
inline int stream_wait_event(void *s, event_t e)
{
	DM_CHECK(hipStreamWaitEvent((hipStream_t)s, e, 0));
	return 0;
}
inline int event_sync(event_t e)
{
	DM_CHECK(hipEventSynchronize(e));
	return 0;
}
#undef DM_CHECK
#else
// ---- host emulation (tests/emu): one device of one compute unit, any ordinal, plain heap memory ----
inline int device_count() { return 1 << 20; }
inline int init(int, int *cus)
{
	*cus = 1;
	return 0;
}
inline int use(int) { return 0; }
inline void enable_peer(int, int) {}
inline int alloc(void **p, size_t bytes)
{
	*p = calloc(bytes ? bytes : 16, 1);
	return *p ? 0 : rfwhip_internal_set_error(RFWHIP_ERR_HIP, "out of memory");
}
inline void mem_info(size_t *free_b, size_t *total_b) { *free_b = *total_b = ~(size_t)0; }
inline int last_launch_error() { return 0; }
#if defined(RFWHIP_EMU_STREAMS) && RFWHIP_EMU_STREAMS
// ---- deferred streams (the _streams variant): emu_streams.h schedules every operation ----
inline void release(void *p)
{
	if (!p)
		return;
	emu_streams::sync_all(); // (hipFree synchronises the device)
	free(p);
}
inline int h2d(void *d, const void *h, size_t n, void *s)
{
	if (n)
		emu_streams::h2d(d, h, n, s);
	return 0;
}
inline int d2d(void *dst, const void *src, size_t n, void *s)
{
	if (n)
		emu_streams::copy(dst, src, n, s);
	return 0;
}
inline int d2h_async(void *h, const void *d, size_t n, void *s) { return d2d(h, d, n, s); }
inline int zero(void *d, size_t n, void *s)
{
	if (n)
		emu_streams::enqueue(s, [d, n]() { memset(d, 0, n); });
	return 0;
}
inline int sync(void *s)
{
	emu_streams::sync(s);
	return 0;
}
inline int stream_create(void **s)
{
	*s = emu_streams::stream_create();
	return 0;
}
inline void stream_destroy(void *s)
{
	if (s)
		emu_streams::stream_destroy(s);
}
typedef emu_streams::Event *event_t;
inline int event_create(event_t *e, bool = true)
{
	*e = emu_streams::event_create();
	return 0;
}
inline void event_destroy(event_t e) { emu_streams::destroy_event(e); }
inline int event_record(event_t &e, void *s)
{
	emu_streams::record(e, s);
	return 0;
}
inline float event_ms(event_t a, event_t b) { return emu_streams::elapsed_ms(a, b); }
inline int stream_wait_event(void *s, event_t e)
{
	emu_streams::wait_event(s, e);
	return 0;
}
inline int event_sync(event_t e)
{
	emu_streams::sync_event(e);
	return 0;
}
#else
// ---- "streams" are immediate: every operation runs when the host issues it ----
inline void release(void *p) { free(p); }
inline int h2d(void *d, const void *h, size_t n, void *)
{
	memcpy(d, h, n);
	return 0;
}
inline int d2d(void *dst, const void *src, size_t n, void *)
{
	memmove(dst, src, n);
	return 0;
}
inline int d2h_async(void *h, const void *d, size_t n, void *)
{
	memcpy(h, d, n);
	return 0;
}
inline int zero(void *d, size_t n, void *)
{
	memset(d, 0, n);
	return 0;
}
inline int sync(void *) { return 0; }
inline int stream_create(void **s)
{
	*s = nullptr;
	return 0;
}
inline void stream_destroy(void *) {}
typedef std::chrono::steady_clock::time_point event_t;
inline int event_create(event_t *, bool = true) { return 0; }
inline void event_destroy(event_t) {}
inline int event_record(event_t &e, void *)
{
	e = std::chrono::steady_clock::now();
	return 0;
}
inline float event_ms(event_t a, event_t b) { return std::chrono::duration<float, std::milli>(b - a).count(); }
inline int stream_wait_event(void *, event_t) { return 0; }
inline int event_sync(event_t) { return 0; }
#endif
inline int host_alloc(void **p, size_t bytes) { return alloc(p, bytes); }
inline void host_free(void *p) { release(p); }
inline int copy_async(void *dst, int, const void *src, int, size_t n, void *s) { return d2d(dst, src, n, s); }
#endif

// a read back the host may use when the call returns: the copy, then a synchronisation of its stream
inline int d2h(void *h, const void *d, size_t n, void *s)
{
	if (!n)
		return 0;
	const int rc = d2h_async(h, d, n, s);
	return rc ? rc : sync(s);
}
} // namespace dm
