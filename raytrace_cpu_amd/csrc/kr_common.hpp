// kr_common.hpp -- host-side plumbing shared by the .hip translation units of libkrtrace.so, and the one wave reduction that the trace loop and the passes share.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <functional>
#include <string>
#include <vector>

#include "../../include/kr_trace.h"

namespace kr {

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what, const char* file, int line);
int require_device();   // KR_OK or KR_ENODEVICE (message set)
// a refused argument: the message "<who>: <what>", KR_EINVAL
inline int invalid_arg(const char* who, const char* what) { set_error(std::string(who) + ": " + what); return KR_EINVAL; }
// KR_V_PLUNGE (include/kr_trace.h): refused where the flow is not built, and taken with motion = 0 alone where it is
inline int refuse_plunge(double V, const char* who) { return V == KR_V_PLUNGE ? invalid_arg(who, "V = KR_V_PLUNGE (the plunging disc flow) is not supported here") : (int) KR_OK; }
inline int accept_plunge(double V, int motion, const char* who)
{
    return V == KR_V_PLUNGE && motion != 0 ? invalid_arg(who, "V = KR_V_PLUNGE (the plunging disc flow) needs motion = 0") : (int) KR_OK;
}
inline bool positive_finite(double x) { return x > 0 && std::isfinite(x); }

#define KR_HIP(call)                                                      \
    do {                                                                  \
        hipError_t e__ = (call);                                          \
        if (e__ != hipSuccess) return kr::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

// device side: the sum of v over the 64 lanes of a wave, in lane 0 (the trace loop's counters, the caustic passes' counts)
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// The current device, saved on construction and set again on destruction: for code that visits other devices (the shutdown paths).
struct CurrentDeviceGuard {
    int saved = 0;
    bool have = false;
    CurrentDeviceGuard() { have = hipGetDevice(&saved) == hipSuccess; (void) hipGetLastError(); }
    CurrentDeviceGuard(const CurrentDeviceGuard&) = delete;
    CurrentDeviceGuard& operator=(const CurrentDeviceGuard&) = delete;
    ~CurrentDeviceGuard() { if (have) (void) hipSetDevice(saved); (void) hipGetLastError(); }
};

// RAII device scratch used by the host-buffer entry points
struct DeviceBuffer {
    void* p = nullptr;
    ~DeviceBuffer() { if (p) (void) hipFree(p); }
    int alloc(size_t bytes);
    int alloc_zeroed(size_t bytes);                  // alloc, then a blocking memset
    int upload(const void* host, size_t bytes);      // alloc, then a blocking copy of host[0 .. bytes); host == null: nothing, p stays null
};

// ---- small constant tables that the host builds and the passes read on the device (the PointSource angle tables, the line emissivity tables) ----
// One device array per distinct (device, kind, key), built by the first lookup that needs it: fill() writes the host contents, then a hipMalloc and
// a blocking copy.  Every lookup pins its entry until the TablePins it was made through goes out of scope: keep that alive until the kernels that
// read the arrays have been enqueued.  When a device holds kMaxDeviceTables entries (kr_capi.hip), a miss drains that device and frees its unpinned
// entries: a kernel that reads one was enqueued before its pin was released, so the drain has finished it.  Pinned entries and other devices'
// entries are never freed by a lookup; while every entry is pinned the count may exceed the cap.
enum TableKind { kAngleTable, kLineTable, kSpectrumKtTable, kSpectrumEmisTable, kSpectrumTable, kResponseTimeTable, kIllumEmisTable, kIllumTimeTable };
// key of kAngleTable: (alpha / beta, x0, dx, n); of kLineTable: the table's bytes, columns; of the three of kr_spectrum.hip (kT and emissivity by
// radius, the rest-frame spectrum S) and of kr_response.hip's source->disc time by radius: the table's bytes; of the two planes of a kr_illum_table: the plane's bytes
struct DeviceTable;
class TablePins {
public:
    TablePins() = default;
    TablePins(const TablePins&) = delete;                  // each pin is released once
    TablePins& operator=(const TablePins&) = delete;
    ~TablePins();
    // *out: the current device's copy of the table (kind, key); key: bytes that determine the contents
    int lookup(TableKind kind, const std::string& key, const std::function<void(std::vector<double>&)>& fill, const double** out);
private:
    std::vector<DeviceTable*> held_;
};
void device_tables_shutdown();     // per device that has tables: drain it, free what no call holds; the caller's device is restored

// device-pointer implementations of the trace (kr_trace.hip); stream may be null.  The passes around it are declared in kr_pass.hpp.
int trace_dev(const kr_params* p, void* d_rays, int64_t n, hipStream_t stream, kr_stats* stats, bool f32);
int trace_async(const kr_params* p, void* d_rays, int64_t n, hipStream_t stream, bool f32, void** ticket);
int trace_batch_async(int count, const kr_params* const* p, void* const* d_rays, const int64_t* n, void* const* streams, void** tickets);
int trace_wait(void* ticket, kr_stats* stats);
int trace_poll(void* ticket, int64_t* rays_started, int32_t* finished);
void trace_release(void* ticket);
void side_stream_forget(hipStream_t user);
int trace_shutdown();
int validate_run(const kr_params* p, const char* who);   // integrator / stop_kind / Euler-with-destination; message "<who>: ..."
int device_cus(int dev, int* cus);
void angle_values(int kind, double x0, double dx, int n, double* sincos_pairs);     // kr_post.hip; kind 0: x = cos(alpha); 1: x = beta

}  // namespace kr
