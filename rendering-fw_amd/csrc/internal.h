// internal.h — what the translation units of librfwhip.so share besides the public C ABI (not installed, not exported).
#pragma once

// sets the calling thread's rfwhip_last_error() text and returns `code` (rfwhip_api.cpp)
int rfwhip_internal_set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// the root's side of a group / comm gather: denoise the full image on `hip_stream` in place when the context's "denoise" is on
// (rfwhip_api.cpp; a no-op otherwise)
struct rfwhip_context;
int rfwhip_internal_denoise_stream(rfwhip_context *ctx, void *rgba_device, void *hip_stream);
