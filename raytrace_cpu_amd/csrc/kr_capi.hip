// kr_capi.hip -- the extern "C" surface declared in include/kr_trace.h.
// Host-pointer entry points stage rays through a private device buffer (H2D, kernels, D2H) so that the
// caller's rays[] is up to date on return, which is the contract of the reference's member functions.
// There is no CPU implementation behind any of these: without a HIP device they return KR_ENODEVICE.

#include <hip/hip_runtime.h>

#include <atomic>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kr_pass.hpp"

namespace kr {

static thread_local std::string g_error;

// (hardware queues: include/kr_trace.h, kr_configure_process -- the library no longer edits the environment when it is loaded)
static std::atomic<bool> g_runtime_touched{false};     // any entry point that reaches the HIP runtime sets it
// (Nothing is released from a library destructor: at process exit the HIP runtime's own exit handlers may already have run -- they are
// registered when the runtime starts, i.e. after this library's -- and calling into a torn-down runtime can hang.  kr_shutdown() is explicit.)

void set_error(const std::string& msg) { g_error = msg; }

int hip_fail(hipError_t e, const char* what, const char* file, int line)
{
    char buf[512];
    std::snprintf(buf, sizeof(buf), "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    g_error = buf;
    (void) hipGetLastError();
    return (e == hipErrorOutOfMemory) ? KR_ENOMEM : (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? KR_ENODEVICE : KR_EHIP;
}

int require_device()
{
    g_runtime_touched = true;
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void) hipGetLastError();
        g_error = "no HIP device available (libkrtrace has no CPU fallback)";
        return KR_ENODEVICE;
    }
    return KR_OK;
}

int DeviceBuffer::alloc(size_t bytes)
{
    KR_HIP(hipMalloc(&p, bytes ? bytes : 1));
    return KR_OK;
}

int DeviceBuffer::alloc_zeroed(size_t bytes)
{
    const int rc = alloc(bytes);
    if (rc != KR_OK) return rc;
    KR_HIP(hipMemset(p, 0, bytes));
    return KR_OK;
}

int DeviceBuffer::upload(const void* host, size_t bytes)
{
    if (!host) return KR_OK;
    const int rc = alloc(bytes);
    if (rc != KR_OK) return rc;
    KR_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    return KR_OK;
}

// ---- the device table store (kr_common.hpp, TablePins) --------------------------------------------------------------------------------
struct DeviceTable { double* d; int pins; };

namespace {
constexpr size_t kMaxDeviceTables = 256;                                // per device, both kinds together
using TableMap = std::map<std::pair<int, std::string>, DeviceTable>;     // (kind, key) -> array
std::mutex g_tables_mu;
std::map<int, TableMap> g_tables;                                       // per device

void free_unpinned(TableMap& tables)                                    // after draining their device
{
    for (auto it = tables.begin(); it != tables.end();) {
        if (it->second.pins) { ++it; continue; }
        (void) hipFree(it->second.d);
        it = tables.erase(it);
    }
}
}  // namespace

int TablePins::lookup(TableKind kind, const std::string& key, const std::function<void(std::vector<double>&)>& fill, const double** out)
{
    int dev = 0;
    KR_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_tables_mu);
    auto& tables = g_tables[dev];
    const auto k = std::make_pair((int) kind, key);
    auto it = tables.find(k);
    if (it == tables.end()) {
        if (tables.size() >= kMaxDeviceTables) {          // full: drain this device, then free what no call holds
            KR_HIP(hipDeviceSynchronize());
            free_unpinned(tables);
        }
        std::vector<double> h;
        fill(h);
        double* d = nullptr;
        KR_HIP(hipMalloc((void**) &d, h.size() * sizeof(double)));
        const hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void) hipFree(d); return hip_fail(e, "hipMemcpy(device table)", __FILE__, __LINE__); }
        it = tables.emplace(k, DeviceTable{d, 0}).first;
    }
    it->second.pins++;
    held_.push_back(&it->second);
    *out = it->second.d;
    return KR_OK;
}

TablePins::~TablePins()
{
    if (held_.empty()) return;
    std::lock_guard<std::mutex> lk(g_tables_mu);
    for (DeviceTable* t : held_) t->pins--;
}

void device_tables_shutdown()
{
    CurrentDeviceGuard restore;
    std::lock_guard<std::mutex> lk(g_tables_mu);
    for (auto& dt : g_tables) {
        if (dt.second.empty()) continue;
        if (hipSetDevice(dt.first) != hipSuccess) { (void) hipGetLastError(); continue; }
        (void) hipDeviceSynchronize();
        free_unpinned(dt.second);
    }
}

namespace {

int invalid(const char* what) { set_error(what); return KR_EINVAL; }

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// ---- attached host arrays ----------------------------------------------------------------------------------------------
// A caller that keeps ONE host ray array through several passes (the class API: Raytracer<T>::rays lives as long as the object)
// attaches it once: a device buffer of the same size is kept for it, and every host-pointer entry point called on it (a) allocates
// nothing, (b) copies back only the bytes its pass modifies -- one 8-byte field per record for redshift_start / range_phi /
// redshift -- through a compact buffer: field-gather kernel, 8 n bytes over PCIe, scatter into rays[] by host threads.
// (Page-locking the array in place with hipHostRegister was measured and dropped: transfers do reach 57 GB/s, but registering
// 1.44 GB costs ~60 ms, the first transfer out of it 140 ms, unregistering ~100 ms -- more than four passes save;
// the runtime's own path for pageable memory already runs at 30-55 GB/s after the first touch: profiles/r02_app_wall.txt.)
// The host array is still the input of every call (it is uploaded each time: an application may have written to it) and is
// complete when the call returns, which is the reference's contract.
struct Attached {
    void* host = nullptr;
    int64_t n = 0;
    size_t ray_bytes = 0;
    void* dev = nullptr;          // n * ray_bytes
    void* d_field = nullptr;      // n * 32: the widest partial write-back (four momenta)
    void* h_field = nullptr;      // host side of it
};
std::mutex g_att_mu;
std::map<const void*, Attached> g_attached;

__global__ void __launch_bounds__(kBlock) gather_field_kernel(const char* __restrict__ rays, long long n, int ray_bytes, int off, int words, double* __restrict__ out)
{
    KR_GRID_STRIDE(i, n) {
        const double* src = reinterpret_cast<const double*>(rays + i * ray_bytes + off);
        for (int w = 0; w < words; w++) out[i * words + w] = src[w];
    }
}

void scatter_field_host(char* rays, int64_t n, size_t ray_bytes, int off, int words, const double* field)
{
    const int nthreads = (int) std::max<int64_t>(1, std::min<int64_t>(8, n / 65536));
    auto work = [&](int t) {
        const int64_t lo = n * t / nthreads, hi = n * (t + 1) / nthreads;
        for (int64_t i = lo; i < hi; i++) std::memcpy(rays + i * ray_bytes + off, field + i * words, (size_t) words * 8);
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
}

// what a pass writes into the records it was given
struct WriteBack {
    int off = 0;         // byte offset of the modified field(s) inside a record
    int words = 0;       // 8-byte words; 0 = the whole record
};
constexpr WriteBack kWholeRecord = {0, 0};

// what a host-pointer call moves: the records up before its kernels run, and which part of them back afterwards
struct Staging {
    bool copy_in, copy_out;
    WriteBack wb;
};
constexpr Staging kConstructs = {false, true, kWholeRecord};      // a source constructor: nothing to upload, every record comes back
constexpr Staging kUpdates = {true, true, kWholeRecord};          // a pass over existing records
constexpr Staging kReads = {true, false, kWholeRecord};           // a reducer: its result leaves by another way
constexpr Staging updates_field(int off, int words) { return {true, true, {off, words}}; }

// the attached array that holds rays[0 .. n), as a whole or as a sub-range (the single-ray propagate() forms pass &rays[i]); .dev is null if none does
Attached find_attached(const void* rays, int64_t n, size_t ray_bytes)
{
    std::lock_guard<std::mutex> lk(g_att_mu);
    auto it = g_attached.upper_bound(rays);
    if (it == g_attached.begin()) return Attached{};
    const Attached& a = (--it)->second;
    const char* base = (const char*) a.host;
    const char* p = (const char*) rays;
    const bool holds = a.ray_bytes == ray_bytes && p >= base && p + (size_t) n * ray_bytes <= base + (size_t) a.n * ray_bytes && (size_t) (p - base) % ray_bytes == 0;
    return holds ? a : Attached{};
}

void release_buffers(const Attached& a)
{
    if (a.dev) (void) hipFree(a.dev);
    if (a.d_field) (void) hipFree(a.d_field);
    std::free(a.h_field);
}

// run `body(d_rays)` on a device copy of a host ray array and copy the result back
template <typename Body>
int with_staged_rays(void* rays, int64_t n, size_t ray_bytes, Staging how, kr_stats* stats, Body body)
{
    if (n < 0 || (n > 0 && !rays)) return invalid("null rays pointer or negative n");
    int rc = require_device();
    if (rc != KR_OK) return rc;
    if (n == 0) return body(nullptr);
    static const bool timing = getenv("KR_TIMING") != nullptr;      // per-call breakdown on stderr (scripts/app_wall.sh)
    const Attached att = find_attached(rays, n, ray_bytes);
    const WriteBack wb = how.wb;
    auto t0 = clk::now();
    DeviceBuffer buf;
    char* d = nullptr;
    if (att.dev) {
        d = (char*) att.dev + ((const char*) rays - (const char*) att.host);
    } else {
        rc = buf.alloc((size_t) n * ray_bytes);
        if (rc != KR_OK) return rc;
        d = (char*) buf.p;
    }
    const double t_alloc = ms_since(t0);
    t0 = clk::now();
    if (how.copy_in) KR_HIP(hipMemcpy(d, rays, (size_t) n * ray_bytes, hipMemcpyHostToDevice));
    const double h2d = ms_since(t0);
    t0 = clk::now();
    rc = body((void*) d);
    if (rc != KR_OK) return rc;
    KR_HIP(hipDeviceSynchronize());
    const double t_body = ms_since(t0);
    t0 = clk::now();
    if (how.copy_out) {
        if (att.dev && wb.words > 0 && wb.words <= 4 && n >= 4096) {
            hipLaunchKernelGGL(gather_field_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, nullptr, (const char*) d, (long long) n,
                               (int) ray_bytes, wb.off, wb.words, (double*) att.d_field);
            KR_HIP(hipGetLastError());
            KR_HIP(hipMemcpy(att.h_field, att.d_field, (size_t) n * wb.words * 8, hipMemcpyDeviceToHost));
            scatter_field_host((char*) rays, n, ray_bytes, wb.off, wb.words, (const double*) att.h_field);
        } else {
            KR_HIP(hipMemcpy(rays, d, (size_t) n * ray_bytes, hipMemcpyDeviceToHost));
        }
    }
    const double d2h = ms_since(t0);
    if (stats) { stats->h2d_ms = h2d; stats->d2h_ms = d2h; }
    if (timing) std::fprintf(stderr, "kr_timing: staged call n=%lld%s alloc %.1f ms h2d %.1f ms kernels %.1f ms d2h %.1f ms%s\n", (long long) n, att.dev ? " (attached)" : "",
                             t_alloc, h2d, t_body, d2h, (att.dev && wb.words > 0) ? " (one field)" : "");
    return KR_OK;
}

// the shape of a device-pointer entry point: its argument check (ok, or `what` is the error), then a device, then the launcher
template <typename Launch>
int on_device(bool ok, const char* what, Launch launch)
{
    if (!ok) return invalid(what);
    const int rc = require_device();
    return rc != KR_OK ? rc : launch();
}

// the shape of a host reducer: the rays staged, `words` zeroed doubles on the device, reduce(d_rays, d_acc) adds into them, they come back into h
template <typename Reduce>
int reduce_to_host(const kr_ray_f64* rays, int64_t n, size_t words, double* h, Reduce reduce)
{
    return with_staged_rays((void*) rays, n, sizeof(kr_ray_f64), kReads, nullptr, [&](void* d) {
        DeviceBuffer acc;
        int rc = acc.alloc_zeroed(words * sizeof(double));
        if (rc != KR_OK) return rc;
        rc = reduce(d, acc.p);
        if (rc != KR_OK) return rc;
        KR_HIP(hipMemcpy(h, acc.p, words * sizeof(double), hipMemcpyDeviceToHost));
        return (int) KR_OK;
    });
}

// the counters of one trace into those of several: sums, and the LARGEST of the durations and of the longest rays (include/kr_trace.h, kr_trace_wait_many)
void accumulate_stats(kr_stats* total, const kr_stats& st)
{
    total->rays_total += st.rays_total; total->rays_traced += st.rays_traced; total->steps_total += st.steps_total;
    total->rk45_attempts += st.rk45_attempts; total->rk45_rejects += st.rk45_rejects; total->rays_strict_side += st.rays_strict_side;
    total->rk45_stationary_steps += st.rk45_stationary_steps; total->rk45_extrapolated_steps += st.rk45_extrapolated_steps;
    total->steps_strict_side += st.steps_strict_side; total->rk45_evaluated_strict_side += st.rk45_evaluated_strict_side;
    total->kernel_ms = std::max(total->kernel_ms, st.kernel_ms);
    total->strict_side_ms = std::max(total->strict_side_ms, st.strict_side_ms);
    total->main_ms = std::max(total->main_ms, st.main_ms);
    total->longest_ray_steps = std::max(total->longest_ray_steps, st.longest_ray_steps);
    total->longest_ray_steps_strict_side = std::max(total->longest_ray_steps_strict_side, st.longest_ray_steps_strict_side);
}


// run_raytrace with show_progress != 0 (raytracer.cpp:84-85, :107-115): the same trace, and while it runs the calling thread polls the work
// queue and reports every multiple of `every` rays it sees passed
int trace_with_progress(const kr_params* p, void* d, int64_t n, bool f32, kr_stats* stats, int64_t every, kr_progress_fn fn, void* user)
{
    void* ticket = nullptr;
    int rc = trace_async(p, d, n, nullptr, f32, &ticket);
    if (rc != KR_OK) return rc;
    int64_t shown = 0;
    for (;;) {
        int64_t started = 0;
        int32_t fin = 1;
        rc = trace_poll(ticket, &started, &fin);
        if (rc != KR_OK) break;                       // (the trace itself is still waited for below)
        if (fn && every > 0) {
            const int64_t at = started / every * every;
            if (at > shown) { shown = at; fn(at, n, user); }
        }
        if (fin) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
    const int rc2 = trace_wait(ticket, stats);
    if (stats) stats->rays_total = n;
    return rc != KR_OK ? rc : rc2;
}

// the four host-pointer traces: params checked, counters cleared, then the trace on the staged records
template <typename Trace>
int trace_host(const kr_params* p, void* rays, int64_t n, size_t ray_bytes, kr_stats* stats, Trace trace)
{
    if (!p) return invalid("kr_trace: null params");
    const int rc = validate_run(p, "kr_trace");          // (before any device work, as the device-pointer forms do: a bad kr_params is KR_EINVAL on every machine)
    if (rc != KR_OK) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return with_staged_rays(rays, n, ray_bytes, kUpdates, stats, trace);
}

}  // namespace
}  // namespace kr

using namespace kr;

extern "C" {

int kr_abi_version(void) { return KR_ABI_VERSION; }
const char* kr_last_error(void) { return g_error.c_str(); }

int kr_device_count(void)
{
    int n = 0;
    g_runtime_touched = true;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void) hipGetLastError();
        set_error("no HIP device available");
        return KR_ENODEVICE;
    }
    return n;
}

int kr_set_device(int device)
{
    KR_HIP(hipSetDevice(device));
    return KR_OK;
}

int kr_device_info(int* cus, int* clock_khz, int64_t* hbm_bytes, char* name, int name_len)
{
    int rc = require_device();
    if (rc != KR_OK) return rc;
    int dev = 0;
    KR_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    KR_HIP(hipGetDeviceProperties(&prop, dev));
    if (cus) *cus = prop.multiProcessorCount;
    if (clock_khz) *clock_khz = prop.clockRate;
    if (hbm_bytes) *hbm_bytes = (int64_t) prop.totalGlobalMem;
    if (name && name_len > 0) {
        std::snprintf(name, (size_t) name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    return KR_OK;
}

// Raytracer<T> ctor defaults, raytracer.cpp:12-22 + raytracer.h:19-44; horizon = kerr_horizon(spin), kerr.h:14-20
void kr_params_default(kr_params* p, double spin)
{
    std::memset(p, 0, sizeof(*p));
    p->spin = spin;
    p->horizon = 1 + std::sqrt((1 - spin) * (1 + spin));
    p->precision = KR_PRECISION;
    p->theta_precision = KR_THETA_PRECISION;
    p->max_tstep = KR_MAXDT;
    p->maxtstep_rlim = KR_MAXDT_RLIM;
    p->max_phistep = KR_MAXDPHI;
    p->rk45_tol = 1e-8;
    p->r_max = 1000;
    p->theta_max = 1.57079632679489661923;
    p->integrator = KR_EULER;
    p->stop_kind = KR_STOP_THETA;
    p->steplim = -1;
}

// src/include/kerr.h:14-20
double kr_kerr_horizon(double a) { return 1 + std::sqrt((1 - a) * (1 + a)); }

// src/include/kerr.h:23-32: A and B are `const float`, and with `using namespace std` in force the last sqrt
// is the float overload, so the ISCO radius the apps bin against is a float-precision number
// (r_isco(0.998) = 1.2369706630706787).  Reproduced, not fixed: it is a bin edge.
double kr_kerr_isco(double a, int sign)
{
    const float A = (float) (1. + std::pow(1. - a * a, 1. / 3.) * (std::pow(1. + a, 1. / 3.) + std::pow(1. - a, 1. / 3.)));
    const float AA = A * A;
    const float B = (float) std::sqrt(3. * a * a + AA);
    const float inner = (3 - A) * (3 + A + 2 * B);
    const float res = 3 + B - sign * std::sqrt(inner);
    return res;
}

// src/include/kerr.h:35-38
double kr_disc_velocity(double r, double a, int sign) { return 1 / (a + sign * std::pow(r, 3. / 2.)); }

// ---- the disc flow of KR_V_PLUNGE (include/kr_trace.h): what the passes hand their kernels, and its four-velocity on the equatorial plane in the
//      expressions of kr_post_device.hpp (plunge_velocity inside r_ms; the e_t of redshift_value with V = 1 / (a + r sqrt(r)) outside) ----
int kr_plunge_flow(double a, double* r_ms, double* E_ms, double* L_ms)
{
    if (!r_ms || !E_ms || !L_ms) return invalid("kr_plunge_flow: null argument");
    if (!(std::fabs(a) <= 1)) return invalid("kr_plunge_flow: |a| must not exceed 1");
    const DiscFlow<true> fl = plunge_flow(a, 0);
    *r_ms = fl.r_ms; *E_ms = fl.E_ms; *L_ms = fl.L_ms;
    return KR_OK;
}

int kr_plunge_velocity(double a, double r, double u[4])
{
    if (!u) return invalid("kr_plunge_velocity: null argument");
    if (!(std::fabs(a) <= 1)) return invalid("kr_plunge_velocity: |a| must not exceed 1");
    if (!std::isfinite(r) || !(r > kr_kerr_horizon(a))) return invalid("kr_plunge_velocity: r must be finite and outside the horizon");
    const DiscFlow<true> fl = plunge_flow(a, 0);
    if (r < fl.r_ms) {
        const double delta = r * r - 2 * r + a * a;
        const double k = fl.E_ms, h = fl.L_ms;
        const double rad = k * k - 1 + 2 / r + (a * a * (k * k - 1) - h * h) / (r * r) + 2 * (h - a * k) * (h - a * k) / (r * r * r);
        u[0] = ((r * r + a * a + 2 * a * a / r) * k - 2 * a * h / r) / delta;
        u[1] = -1 * std::sqrt(rad > 0 ? rad : 0.0);
        u[2] = 0;
        u[3] = (2 * a * k / r + (1 - 2 / r) * h) / delta;
    } else {
        // the metric on the plane itself (sin = 1, cos = 0), kerr_metric's expressions
        const double rhosq = r * r, delta = r * r - 2 * r + a * a;
        const double sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta;
        const double e2nu = rhosq * delta / sigmasq, e2psi = sigmasq / rhosq, omega = 2 * a * r / sigmasq;
        const double V = 1 / (a + r * std::sqrt(r));
        u[0] = (1 / std::sqrt(e2nu)) / std::sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
        u[1] = 0;
        u[2] = 0;
        u[3] = (1 / std::sqrt(e2nu)) * V / std::sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
    }
    return KR_OK;
}

// nRays is the int-truncated PRODUCT of doubles (pointsource.cpp:12), n_cosalpha / n_beta the truncated factors (:16-17)
int64_t kr_pointsource_count(const kr_pointsource* s, int32_t* n_cosalpha, int32_t* n_beta)
{
    const int nrays = (int) ((((s->cosalphamax - s->cosalpha0) / s->dcosalpha) + 1) * (((s->betamax - s->beta0) / s->dbeta) + 1));
    if (n_cosalpha) *n_cosalpha = (int) (((s->cosalphamax - s->cosalpha0) / s->dcosalpha) + 1);
    if (n_beta) *n_beta = (int) (((s->betamax - s->beta0) / s->dbeta) + 1);
    return nrays;
}

// What the device PointSource constructor reads instead of calling acos / sin / cos / tan itself (kr_post_device.hpp::SourceTables): host values.
int kr_pointsource_tables(const kr_pointsource* s, double* alpha_sincos, double* beta_sincos, double* pos_sin_cos_tan)
{
    if (!s) return invalid("kr_pointsource_tables: null spec");
    int32_t nc = 0, nb = 0;
    kr_pointsource_count(s, &nc, &nb);
    if (alpha_sincos) angle_values(0, s->cosalpha0, s->dcosalpha, nc, alpha_sincos);
    if (beta_sincos) angle_values(1, s->beta0, s->dbeta, nb, beta_sincos);
    if (pos_sin_cos_tan) { ::sincos(s->pos[2], &pos_sin_cos_tan[0], &pos_sin_cos_tan[1]); pos_sin_cos_tan[2] = std::tan(s->pos[2]); }
    return KR_OK;
}

// imageplane.cpp:12-14
int64_t kr_imageplane_count(const kr_imageplane* s, int32_t* nx, int32_t* ny)
{
    const int nrays = (int) ((((s->xmax - s->x0) / s->dx) + 1) * (((s->ymax - s->y0) / s->dy) + 1));
    if (nx) *nx = (int) (((s->xmax - s->x0) / s->dx) + 1);
    if (ny) *ny = (int) (((s->ymax - s->y0) / s->dy) + 1);
    return nrays;
}

// imageplane_bundles.h:150-153: the Raytracer allocation, five times the int-truncated product of doubles
int64_t kr_bundles_count(const kr_imageplane* s, int32_t* nx, int32_t* ny)
{
    return 5 * kr_imageplane_count(s, nx, ny);
}

// ---- trace ---------------------------------------------------------------------------------------------
int kr_trace_dev_f64(const kr_params* p, void* d_rays, int64_t n, void* stream, kr_stats* stats)
{
    return trace_dev(p, d_rays, n, (hipStream_t) stream, stats, false);
}

int kr_trace_dev_f32(const kr_params* p, void* d_rays, int64_t n, void* stream, kr_stats* stats)
{
    return trace_dev(p, d_rays, n, (hipStream_t) stream, stats, true);
}

int kr_trace_async_f64(const kr_params* p, void* d_rays, int64_t n, void* stream, void** ticket)
{
    return ticket ? trace_async(p, d_rays, n, (hipStream_t) stream, false, ticket) : invalid("kr_trace_async: null ticket pointer");
}

int kr_trace_async_f32(const kr_params* p, void* d_rays, int64_t n, void* stream, void** ticket)
{
    return ticket ? trace_async(p, d_rays, n, (hipStream_t) stream, true, ticket) : invalid("kr_trace_async: null ticket pointer");
}

int kr_trace_batch_async_f64(int32_t count, const kr_params* const* p, void* const* d_rays, const int64_t* n, void* const* streams, void** tickets)
{
    return trace_batch_async(count, p, d_rays, n, streams, tickets);
}

int kr_trace_wait(void* ticket, kr_stats* stats) { return trace_wait(ticket, stats); }

int kr_trace_wait_many(int32_t count, void* const* tickets, kr_stats* per_ticket, kr_stats* total)
{
    if (count < 0 || (count > 0 && !tickets)) return invalid("kr_trace_wait_many: null argument");
    if (total) std::memset(total, 0, sizeof(*total));
    int first_rc = KR_OK;
    for (int32_t i = 0; i < count; i++) {
        kr_stats st;
        const int rc = trace_wait(tickets[i], (per_ticket || total) ? &st : nullptr);
        if (rc != KR_OK) { if (first_rc == KR_OK) first_rc = rc; continue; }
        if (per_ticket) per_ticket[i] = st;
        if (total) accumulate_stats(total, st);
    }
    return first_rc;
}

int kr_trace_release(void* ticket)
{
    trace_release(ticket);
    return KR_OK;
}

int kr_trace_f64(const kr_params* p, kr_ray_f64* rays, int64_t n, kr_stats* stats)
{
    return trace_host(p, rays, n, sizeof(kr_ray_f64), stats, [&](void* d) { return trace_dev(p, d, n, nullptr, stats, false); });
}
int kr_trace_f32(const kr_params* p, kr_ray_f32* rays, int64_t n, kr_stats* stats)
{
    return trace_host(p, rays, n, sizeof(kr_ray_f32), stats, [&](void* d) { return trace_dev(p, d, n, nullptr, stats, true); });
}
int kr_trace_progress_f64(const kr_params* p, kr_ray_f64* rays, int64_t n, kr_stats* stats, int64_t every, kr_progress_fn fn, void* user)
{
    return trace_host(p, rays, n, sizeof(kr_ray_f64), stats, [&](void* d) { return trace_with_progress(p, d, n, false, stats, every, fn, user); });
}
int kr_trace_progress_f32(const kr_params* p, kr_ray_f32* rays, int64_t n, kr_stats* stats, int64_t every, kr_progress_fn fn, void* user)
{
    return trace_host(p, rays, n, sizeof(kr_ray_f32), stats, [&](void* d) { return trace_with_progress(p, d, n, true, stats, every, fn, user); });
}
int kr_trace_poll(void* ticket, int64_t* rays_started, int32_t* finished)
{
    return trace_poll(ticket, rays_started, finished);
}

// ---- per-step ray paths (kr_paths.hip): the serial branch of run_raytrace, raytracer.cpp:86-100 -------------------------------------------------
// everything is validated before anything touches a device
int kr_trace_paths_count_dev_f64(const kr_params* p, const kr_path_spec* w, const void* d_rays, int64_t n, void* d_offsets, void* d_traced, int64_t* total_rows,
                                 void* stream)
{
    const int rc = paths_validate(p, w, "kr_trace_paths_count");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && (n == 0 || d_rays) && d_offsets && total_rows, "kr_trace_paths_count: null argument or negative n",
                     [&] { return paths_count_dev(p, w, d_rays, n, d_offsets, d_traced, total_rows, (hipStream_t) stream); });
}

int kr_trace_paths_record_dev_f64(const kr_params* p, const kr_path_spec* w, void* d_rays, int64_t n, const void* d_offsets, void* d_rows, int64_t total_rows,
                                  void* stream, kr_stats* stats)
{
    const int rc = paths_validate(p, w, "kr_trace_paths_record");
    if (rc != KR_OK) return rc;
    if (n < 0 || (n > 0 && !d_rays) || !d_offsets || !d_rows || total_rows < 0) return invalid("kr_trace_paths_record: null argument, negative n or negative total_rows");
    if ((uintptr_t) d_rows % 32 != 0) return invalid("kr_trace_paths_record: d_rows must be 32-byte aligned");
    return on_device(true, nullptr, [&] { return paths_record_dev(p, w, d_rays, n, d_offsets, d_rows, total_rows, (hipStream_t) stream, stats); });
}

int kr_trace_paths_f64(const kr_params* p, const kr_path_spec* w, kr_ray_f64* rays, int64_t n, int64_t* offsets, uint8_t* traced, double** rows, int64_t* total_rows,
                       kr_stats* stats)
{
    const int rc = paths_validate(p, w, "kr_trace_paths");
    if (rc != KR_OK) return rc;
    if (!offsets || !rows || !total_rows) return invalid("kr_trace_paths: null argument");
    *rows = nullptr;
    *total_rows = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    void* h_rows = nullptr;               // handed out only when the whole call, copy-back of rays[] included, has succeeded
    int64_t total = 0;
    const int rc_all = with_staged_rays(rays, n, sizeof(kr_ray_f64), kUpdates, stats, [&](void* d) -> int {
        DeviceBuffer d_off, d_traced, d_rows;
        int rc2 = d_off.alloc((size_t) (n + 1) * sizeof(int64_t));
        if (rc2 == KR_OK) rc2 = d_traced.alloc((size_t) n);
        if (rc2 != KR_OK) return rc2;
        rc2 = paths_count_dev(p, w, d, n, d_off.p, d_traced.p, &total, nullptr);
        if (rc2 != KR_OK) return rc2;
        rc2 = d_rows.alloc((size_t) total * 4 * sizeof(double));
        if (rc2 != KR_OK) return rc2;
        rc2 = paths_record_dev(p, w, d, n, d_off.p, d_rows.p, total, nullptr, stats);
        if (rc2 != KR_OK) return rc2;
        KR_HIP(hipHostMalloc(&h_rows, total > 0 ? (size_t) total * 4 * sizeof(double) : 1, hipHostMallocDefault));
        hipError_t e = hipMemcpy(offsets, d_off.p, (size_t) (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess && traced && n > 0) e = hipMemcpy(traced, d_traced.p, (size_t) n, hipMemcpyDeviceToHost);
        if (e == hipSuccess && total > 0) e = hipMemcpy(h_rows, d_rows.p, (size_t) total * 4 * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(paths)", __FILE__, __LINE__);
        return (int) KR_OK;
    });
    if (rc_all != KR_OK) {
        if (h_rows) (void) hipHostFree(h_rows);
        return rc_all;
    }
    *rows = (double*) h_rows;
    *total_rows = total;
    return KR_OK;
}

// ---- volume illumination maps (kr_volume.hip): Mapper::map_ray, mapper.cpp:110-281 ---------------------------------------------------------------
int kr_trace_volume_dev_f64(const kr_params* p, const kr_volume_map* m, void* d_rays, int64_t n, void* d_map, void* stream, kr_stats* stats)
{
    const int rc = volume_validate(p, m, "kr_trace_volume");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && (n == 0 || d_rays) && d_map, "kr_trace_volume: null argument or negative n",
                     [&] { return trace_volume_dev(p, m, d_rays, n, d_map, (hipStream_t) stream, stats); });
}

int kr_trace_volume_f64(const kr_params* p, const kr_volume_map* m, kr_ray_f64* rays, int64_t n, double* map, kr_stats* stats)
{
    const int rc = volume_validate(p, m, "kr_trace_volume");
    if (rc != KR_OK) return rc;
    if (!map || n < 0 || (n > 0 && !rays)) return invalid("kr_trace_volume: null argument or negative n");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const size_t words = 3 * (size_t) m->nr * m->ntheta * m->nphi + 4;
    return with_staged_rays(rays, n, sizeof(kr_ray_f64), kUpdates, stats, [&](void* d) -> int {
        DeviceBuffer d_map;
        int rc2 = d_map.alloc_zeroed(words * sizeof(double));
        if (rc2 != KR_OK) return rc2;
        rc2 = trace_volume_dev(p, m, d, n, d_map.p, nullptr, stats);
        if (rc2 != KR_OK) return rc2;
        KR_HIP(hipMemcpy(map, d_map.p, words * sizeof(double), hipMemcpyDeviceToHost));
        return (int) KR_OK;
    });
}

// ---- equatorial crossings (kr_crossings.hip) and the image of one order from them (kr_post.hip) ----------------------------------------------------
int kr_trace_crossings_dev_f64(const kr_params* p, const kr_crossing_spec* sp, void* d_rays, int64_t n, void* d_rows, void* d_seen, void* stream, kr_stats* stats)
{
    const int rc = crossings_validate(p, sp, "kr_trace_crossings");
    if (rc != KR_OK) return rc;
    if (n < 0 || (n > 0 && !d_rays) || !d_rows || !d_seen) return invalid("kr_trace_crossings: null argument or negative n");
    if ((uintptr_t) d_rows % 32 != 0) return invalid("kr_trace_crossings: d_rows must be 32-byte aligned");
    return on_device(true, nullptr, [&] { return trace_crossings_dev(p, sp, d_rays, n, d_rows, d_seen, (hipStream_t) stream, stats); });
}

int kr_trace_crossings_f64(const kr_params* p, const kr_crossing_spec* sp, kr_ray_f64* rays, int64_t n, double* rows, int32_t* seen, kr_stats* stats)
{
    const int rc = crossings_validate(p, sp, "kr_trace_crossings");
    if (rc != KR_OK) return rc;
    if (n < 0 || (n > 0 && !rays) || !rows || !seen) return invalid("kr_trace_crossings: null argument or negative n");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const size_t row_bytes = (size_t) n * sp->max_crossings * 4 * sizeof(double);
    return with_staged_rays(rays, n, sizeof(kr_ray_f64), kUpdates, stats, [&](void* d) -> int {
        DeviceBuffer d_rows, d_seen;          // (hipMalloc: 256-byte aligned)
        int rc2 = d_rows.upload(rows, row_bytes);
        if (rc2 == KR_OK) rc2 = d_seen.alloc((size_t) n * sizeof(int32_t));
        if (rc2 != KR_OK) return rc2;
        rc2 = trace_crossings_dev(p, sp, d, n, d_rows.p, d_seen.p, nullptr, stats);
        if (rc2 != KR_OK) return rc2;
        if (n > 0) {
            KR_HIP(hipMemcpy(rows, d_rows.p, row_bytes, hipMemcpyDeviceToHost));
            KR_HIP(hipMemcpy(seen, d_seen.p, (size_t) n * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        return (int) KR_OK;
    });
}

int kr_reduce_crossing_image_dev_f64(const kr_image_bins* b, int32_t max_crossings, int32_t order, double lo, double hi, const void* d_rays, const void* d_rows,
                                     const void* d_seen, int64_t n, void* d_planes, void* stream)
{
    if (!b || !d_planes || n < 0 || (n > 0 && (!d_rays || !d_rows || !d_seen))) return invalid("kr_reduce_crossing_image: null argument or negative n");
    if (b->img_nx <= 0 || b->img_ny <= 0) return invalid("kr_reduce_crossing_image: image size must be positive");
    if (max_crossings < 1 || max_crossings > 16) return invalid("kr_reduce_crossing_image: max_crossings must be 1..16");
    if (order < -1 || order >= max_crossings) return invalid("kr_reduce_crossing_image: order must be -1 (the opaque disc) or 0 .. max_crossings - 1");
    return on_device(true, nullptr, [&] { return reduce_crossing_image_dev(b, max_crossings, order, lo, hi, d_rays, d_rows, d_seen, n, d_planes, (hipStream_t) stream); });
}

// ---- observing a volume map (kr_observe.hip): SourceTracer::propagate_source, source_tracer.cpp:102-310 -------------------------------------------
int kr_trace_observe_dev_f64(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const void* d_emis, const void* d_kappa, const void* d_delay,
                             void* d_rays, int64_t n, void* d_out, void* d_image, void* stream, kr_stats* stats)
{
    const int rc = observe_validate(p, m, b, "kr_trace_observe");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && (n == 0 || d_rays) && d_emis && d_out, "kr_trace_observe: null argument (emis, out or rays) or negative n",
                     [&] { return trace_observe_dev(p, m, b, d_emis, d_kappa, d_delay, d_rays, n, d_out, d_image, (hipStream_t) stream, stats); });
}

int kr_trace_observe_f64(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const double* emis, const double* kappa, const double* delay,
                         kr_ray_f64* rays, int64_t n, double* out, double* image, kr_stats* stats)
{
    const int rc = observe_validate(p, m, b, "kr_trace_observe");
    if (rc != KR_OK) return rc;
    if (!emis || !out || n < 0 || (n > 0 && !rays)) return invalid("kr_trace_observe: null argument (emis, out or rays) or negative n");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const size_t ncell = (size_t) m->nr * m->ntheta * m->nphi;
    const size_t words = 2 * (size_t) b->nen + (size_t) b->nen * b->nt + 6;
    return with_staged_rays(rays, n, sizeof(kr_ray_f64), kUpdates, stats, [&](void* d) -> int {
        DeviceBuffer d_out, d_image, d_cells[3];
        const double* h_cells[3] = {emis, kappa, delay};
        int rc2 = d_out.alloc_zeroed(words * sizeof(double));
        for (int q = 0; q < 3 && rc2 == KR_OK; ++q) rc2 = d_cells[q].upload(h_cells[q], ncell * sizeof(double));
        if (rc2 == KR_OK && image && n > 0) rc2 = d_image.alloc((size_t) n * sizeof(double));
        if (rc2 != KR_OK) return rc2;
        rc2 = trace_observe_dev(p, m, b, d_cells[0].p, d_cells[1].p, d_cells[2].p, d, n, d_out.p, d_image.p, nullptr, stats);
        if (rc2 != KR_OK) return rc2;
        KR_HIP(hipMemcpy(out, d_out.p, words * sizeof(double), hipMemcpyDeviceToHost));
        if (d_image.p) KR_HIP(hipMemcpy(image, d_image.p, (size_t) n * sizeof(double), hipMemcpyDeviceToHost));
        return (int) KR_OK;
    });
}

// ---- O(N) passes -------------------------------------------------------------------------------------------
// One line per pass: its scalar arguments, and the field(s) of a kr_ray_f64 it writes.  Each becomes four entry points: device and host
// pointers, for Raytracer<double> and for Raytracer<float> (kr_ray_f32 records, float arithmetic; the scalars are float values carried in
// doubles).  The f64 host form copies back only the written field(s) of an attached array, the f32 host form the whole 84-byte record.
#define KR_LIST(...) __VA_ARGS__
// guard64 / guard32: an int expression over the pass's arguments and `who` (the function's name), evaluated before anything else; a non-zero value is
// returned (KR_V_PLUNGE, include/kr_trace.h)
#define KR_PASS_FORMS(name, T, f32, params, args, staging, guard)                                                     \
    int kr_##name##_dev_##T(KR_LIST params, void* d, int64_t n, void* st)                                             \
    {                                                                                                                 \
        const char* who = f32 ? "kr_" #name "_f32" : "kr_" #name;                                                     \
        if (const int rc = (guard)) return rc;                                                                        \
        return on_device(true, nullptr, [&] { return name##_dev(KR_LIST args, d, n, (hipStream_t) st, f32); });       \
    }                                                                                                                 \
    int kr_##name##_##T(KR_LIST params, kr_ray_##T* rays, int64_t n)                                                  \
    {                                                                                                                 \
        const char* who = f32 ? "kr_" #name "_f32" : "kr_" #name;                                                     \
        if (const int rc = (guard)) return rc;                                                                        \
        return with_staged_rays(rays, n, sizeof(kr_ray_##T), staging, nullptr,                                        \
                                [&](void* d) { return name##_dev(KR_LIST args, d, n, nullptr, f32); });               \
    }
#define KR_PASS(name, params, args, field, words, guard64, guard32)                                              \
    KR_PASS_FORMS(name, f64, false, params, args, updates_field(offsetof(kr_ray_f64, field), words), guard64)    \
    KR_PASS_FORMS(name, f32, true, params, args, kUpdates, guard32)
#define KR_NO_GUARD ((void) who, (int) KR_OK)

KR_PASS(redshift_start, (double spin, double V, int reverse, int projradius), (spin, V, reverse, projradius), emit, 1, refuse_plunge(V, who), refuse_plunge(V, who))
KR_PASS(redshift, (double spin, double V, int reverse, int projradius, int motion), (spin, V, reverse, projradius, motion), redshift, 1, accept_plunge(V, motion, who),
        refuse_plunge(V, who))
KR_PASS(redshift_dest, (double spin, int reverse), (spin, reverse), redshift, 1, KR_NO_GUARD, KR_NO_GUARD)
KR_PASS(range_phi, (double lo, double hi), (lo, hi), phi, 1, KR_NO_GUARD, KR_NO_GUARD)
KR_PASS(calculate_momentum, (double spin), (spin), pt, 4, KR_NO_GUARD, KR_NO_GUARD)

// ---- sources -----------------------------------------------------------------------------------------------
int kr_pointsource_init_dev_f64(const kr_pointsource* s, void* d, int64_t n, void* st)
{
    if (s && refuse_plunge(s->V, "kr_pointsource_init")) return KR_EINVAL;
    return on_device(s, "kr_pointsource_init: null spec", [&] { return pointsource_init_dev(s, d, n, 0, 1, (hipStream_t) st); });
}
int kr_pointsource_init_f64(const kr_pointsource* s, kr_ray_f64* rays, int64_t n)
{
    if (!s) return invalid("kr_pointsource_init: null spec");
    if (refuse_plunge(s->V, "kr_pointsource_init")) return KR_EINVAL;
    return with_staged_rays(rays, n, sizeof(kr_ray_f64), kConstructs, nullptr, [&](void* d) { return pointsource_init_dev(s, d, n, 0, 1, nullptr); });
}

int kr_imageplane_init_dev_f64(const kr_imageplane* s, void* d, int64_t n, void* st)
{
    return on_device(s, "kr_imageplane_init: null spec", [&] { return imageplane_init_dev(s, d, n, 0, 1, (hipStream_t) st); });
}
int kr_imageplane_init_f64(const kr_imageplane* s, kr_ray_f64* rays, int64_t n)
{
    if (!s) return invalid("kr_imageplane_init: null spec");
    return with_staged_rays(rays, n, sizeof(kr_ray_f64), kConstructs, nullptr, [&](void* d) { return imageplane_init_dev(s, d, n, 0, 1, nullptr); });
}

// strided forms: slot k of d_rays receives ray (first + k*stride) of the source's array -- the multi-GPU shard of rank r
// of R is (first = r, stride = R, count = ceil((total - r) / R)); no rank ever materialises another rank's rays.
int kr_pointsource_init_strided_dev_f64(const kr_pointsource* s, int64_t first, int64_t stride, void* d, int64_t count, void* st)
{
    if (s && refuse_plunge(s->V, "kr_pointsource_init_strided")) return KR_EINVAL;
    return on_device(s, "kr_pointsource_init: null spec", [&] { return pointsource_init_dev(s, d, count, first, stride, (hipStream_t) st); });
}
int kr_imageplane_init_strided_dev_f64(const kr_imageplane* s, int64_t first, int64_t stride, void* d, int64_t count, void* st)
{
    return on_device(s, "kr_imageplane_init: null spec", [&] { return imageplane_init_dev(s, d, count, first, stride, (hipStream_t) st); });
}
// fused pipeline ends (device-resident callers): source constructor + redshift_start() in one pass ...
int kr_pointsource_init_emit_dev_f64(const kr_pointsource* s, int64_t first, int64_t stride, double V, int reverse, int projradius, void* d, int64_t count, void* st)
{
    if (refuse_plunge(V, "kr_pointsource_init_emit") || (s && refuse_plunge(s->V, "kr_pointsource_init_emit"))) return KR_EINVAL;
    return on_device(s, "kr_pointsource_init_emit: null spec",
                     [&] { return pointsource_init_emit_dev(s, d, count, first, stride, V, reverse, projradius, (hipStream_t) st); });
}
int kr_pointsource_init_emit_batch_dev_f64(int32_t count, const kr_pointsource* s, const double* V, int reverse, int projradius, void* const* d, const int64_t* n, void* st)
{
    if (count < 0 || (count > 0 && (!s || !d || !n))) return invalid("kr_pointsource_init_emit_batch: null argument");
    for (int32_t i = 0; i < count; i++)
        if (n[i] > 0 && !d[i]) return invalid("kr_pointsource_init_emit_batch: null ray buffer");
    for (int32_t i = 0; i < count; i++)
        if (refuse_plunge(s[i].V, "kr_pointsource_init_emit_batch") || (V && refuse_plunge(V[i], "kr_pointsource_init_emit_batch"))) return KR_EINVAL;
    return on_device(true, nullptr, [&] { return pointsource_init_emit_batch_dev(count, s, V, reverse, projradius, d, n, (hipStream_t) st); });
}
int kr_imageplane_init_emit_dev_f64(const kr_imageplane* s, int64_t first, int64_t stride, double V, int reverse, int projradius, void* d, int64_t count, void* st)
{
    if (refuse_plunge(V, "kr_imageplane_init_emit")) return KR_EINVAL;
    return on_device(s, "kr_imageplane_init_emit: null spec",
                     [&] { return imageplane_init_emit_dev(s, d, count, first, stride, 1, -1 * s->spin, V, reverse, projradius, (hipStream_t) st); });
}
int kr_imageplane_init_emit_runs_dev_f64(const kr_imageplane* s, int64_t first, int64_t stride, int64_t run, double V, int reverse, int projradius, void* d,
                                         int64_t count, void* st)
{
    if (refuse_plunge(V, "kr_imageplane_init_emit_runs")) return KR_EINVAL;
    return on_device(s, "kr_imageplane_init_emit_runs: null spec",
                     [&] { return imageplane_init_emit_dev(s, d, count, first, stride, run, -1 * s->spin, V, reverse, projradius, (hipStream_t) st); });
}
// ... and range_phi() + redshift() + the emissivity histogram / the seven image planes in one pass
int kr_post_emissivity_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_emis_bins* b, void* d, int64_t n,
                               void* d_hist, void* st)
{
    if (accept_plunge(V, motion, "kr_post_emissivity")) return KR_EINVAL;
    return on_device(b && d_hist, "kr_post_emissivity: null argument",
                     [&] { return post_emissivity_dev(spin, V, reverse, projradius, motion, lo, hi, b, d, n, d_hist, (hipStream_t) st); });
}
int kr_post_image_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_image_bins* b, void* d, int64_t n,
                          void* d_planes, void* st)
{
    if (accept_plunge(V, motion, "kr_post_image")) return KR_EINVAL;
    return on_device(b && d_planes, "kr_post_image: null argument",
                     [&] { return post_image_dev(spin, V, reverse, projradius, motion, lo, hi, b, d, n, d_planes, (hipStream_t) st); });
}

// ---- reducers ------------------------------------------------------------------------------------------------
int kr_reduce_emissivity_dev_f64(const kr_emis_bins* b, const void* d, int64_t n, void* d_hist, void* st)
{
    return on_device(b && d_hist, "kr_reduce_emissivity: null argument", [&] { return reduce_emissivity_dev(b, d, n, d_hist, (hipStream_t) st); });
}

int kr_reduce_emissivity_f64(const kr_emis_bins* b, const kr_ray_f64* rays, int64_t n, int64_t* count, double* flux,
                             double* emis, double* sum_redshift, double* sum_time, int64_t* disc_count)
{
    if (!b || !count || !flux || !emis || !sum_redshift || !sum_time) return invalid("kr_reduce_emissivity: null argument");
    if (b->nr <= 0) return invalid("kr_reduce_emissivity: nr must be positive");
    const int nr = b->nr;
    std::vector<double> h((size_t) 5 * nr + 1, 0.0);
    const int rc = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_hist) { return reduce_emissivity_dev(b, d, n, d_hist, nullptr); });
    if (rc != KR_OK) return rc;
    for (int i = 0; i < nr; i++) {
        count[i] = (int64_t) h[i];
        flux[i] = h[nr + i];
        emis[i] = h[2 * nr + i];
        sum_redshift[i] = h[3 * nr + i];
        sum_time[i] = h[4 * nr + i];
    }
    if (disc_count) *disc_count = (int64_t) h[5 * nr];
    return KR_OK;
}

int kr_reduce_image_dev_f64(const kr_image_bins* b, const void* d, int64_t n, void* d_planes, void* st)
{
    return on_device(b && d_planes, "kr_reduce_image: null argument", [&] { return reduce_image_dev(b, d, n, d_planes, (hipStream_t) st); });
}

int kr_reduce_image_f64(const kr_image_bins* b, const kr_ray_f64* rays, int64_t n, int32_t* nrays, double* flux, double* r,
                        double* phi, double* enshift, double* time, double* emis, int64_t* disc_count)
{
    if (!b || !nrays || !flux || !r || !phi || !enshift || !time || !emis) return invalid("kr_reduce_image: null argument");
    if (b->img_nx <= 0 || b->img_ny <= 0) return invalid("kr_reduce_image: image size must be positive");
    const size_t npix = (size_t) b->img_nx * b->img_ny;
    std::vector<double> h(7 * npix + 1, 0.0);
    const int rc = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_planes) { return reduce_image_dev(b, d, n, d_planes, nullptr); });
    if (rc != KR_OK) return rc;
    for (size_t i = 0; i < npix; i++) nrays[i] = (int32_t) h[i];
    double* const planes[] = {flux, r, phi, enshift, time, emis};
    for (size_t k = 0; k < 6; k++) std::memcpy(planes[k], &h[(k + 1) * npix], npix * sizeof(double));
    if (disc_count) *disc_count = (int64_t) h[7 * npix];
    return KR_OK;
}

// the two reducers for rays that ended on a stop surface (kr_surface.hip), and their fused forms
int kr_reduce_emissivity_surface_dev_f64(const kr_emis_bins* b, const void* d, int64_t n, void* d_hist, void* st)
{
    return on_device(b && d_hist && (n <= 0 || d), "kr_reduce_emissivity_surface: null argument", [&] { return reduce_emissivity_surface_dev(b, d, n, d_hist, (hipStream_t) st); });
}
int kr_post_emissivity_surface_dev_f64(double spin, int reverse, double lo, double hi, const kr_emis_bins* b, void* d, int64_t n, void* d_hist, void* st)
{
    return on_device(b && d_hist && (n <= 0 || d), "kr_post_emissivity_surface: null argument",
                     [&] { return post_emissivity_surface_dev(spin, reverse, lo, hi, b, d, n, d_hist, (hipStream_t) st); });
}
int kr_reduce_image_surface_dev_f64(const kr_image_bins* b, const void* d, int64_t n, void* d_planes, void* st)
{
    return on_device(b && d_planes && (n <= 0 || d), "kr_reduce_image_surface: null argument", [&] { return reduce_image_surface_dev(b, d, n, d_planes, (hipStream_t) st); });
}
int kr_post_image_surface_dev_f64(double spin, int reverse, double lo, double hi, const kr_image_bins* b, void* d, int64_t n, void* d_planes, void* st)
{
    return on_device(b && d_planes && (n <= 0 || d), "kr_post_image_surface: null argument",
                     [&] { return post_image_surface_dev(spin, reverse, lo, hi, b, d, n, d_planes, (hipStream_t) st); });
}

int kr_reduce_return_dev_f64(const kr_return_bins* b, const void* d, int64_t n, void* d_out4, void* st)
{
    return on_device(b && d_out4, "kr_reduce_return: null argument", [&] { return reduce_return_dev(b, d, n, d_out4, (hipStream_t) st); });
}

int kr_post_return_dev_f64(double lo, double hi, const kr_return_bins* b, void* d, int64_t n, void* d_out4, void* st)
{
    return on_device(b && d_out4, "kr_post_return: null argument", [&] { return post_return_dev(lo, hi, b, d, n, d_out4, (hipStream_t) st); });
}

int kr_post_return_batch_dev_f64(int32_t count, double lo, double hi, const kr_return_bins* b, void* const* d, const int64_t* n, void* const* d_out4, void* st)
{
    if (count < 0 || (count > 0 && (!b || !d || !n || !d_out4))) return invalid("kr_post_return_batch: null argument");
    for (int32_t i = 0; i < count; i++)
        if (n[i] > 0 && (!d[i] || !d_out4[i])) return invalid("kr_post_return_batch: null buffer");
    return on_device(true, nullptr, [&] { return post_return_batch_dev(count, lo, hi, b, d, n, d_out4, (hipStream_t) st); });
}

int kr_reduce_return_f64(const kr_return_bins* b, const kr_ray_f64* rays, int64_t n, double out[4])
{
    if (!b || !out) return invalid("kr_reduce_return: null argument");
    return reduce_to_host(rays, n, 4, out, [&](void* d, void* d_out4) { return reduce_return_dev(b, d, n, d_out4, nullptr); });
}

// ---- emission line (kr_line.hip): the bins are validated before anything touches a device ----------------------------------
int kr_reduce_return_map_dev_f64(const kr_return_map* m, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = return_map_validate(m, "kr_reduce_return_map");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_return_map: null argument or negative n", [&] { return reduce_return_map_dev(m, d, n, d_out, (hipStream_t) st); });
}

int kr_post_return_map_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_return_map* m, void* d, int64_t n,
                               void* d_out, void* st)
{
    int rc = refuse_plunge(V, "kr_post_return_map");
    if (rc == KR_OK) rc = return_map_validate(m, "kr_post_return_map");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_return_map: null argument or negative n",
                     [&] { return post_return_map_dev(spin, V, reverse, projradius, motion, lo, hi, m, d, n, d_out, (hipStream_t) st); });
}

int kr_post_return_map_batch_dev_f64(int32_t count, double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_return_map* m,
                                     void* const* d, const int64_t* n, void* const* d_out, void* st)
{
    if (refuse_plunge(V, "kr_post_return_map_batch")) return KR_EINVAL;
    if (count < 0 || (count > 0 && (!m || !d || !n || !d_out))) return invalid("kr_post_return_map_batch: null argument or negative count");
    for (int32_t i = 0; i < count; i++) {
        const int rc = return_map_validate(&m[i], "kr_post_return_map_batch");
        if (rc != KR_OK) return rc;
        if (n[i] < 0) return invalid("kr_post_return_map_batch: negative n");
        if (n[i] > 0 && (!d[i] || !d_out[i])) return invalid("kr_post_return_map_batch: null buffer");
    }
    if (count == 0) return KR_OK;
    return on_device(true, nullptr, [&] { return post_return_map_batch_dev(count, spin, V, reverse, projradius, motion, lo, hi, m, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_return_map_f64(const kr_return_map* m, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = return_map_validate(m, "kr_reduce_return_map");
    if (rc != KR_OK) return rc;
    if (!out) return invalid("kr_reduce_return_map: null argument");
    return reduce_to_host(rays, n, 5 * (size_t) m->nr + 6, out, [&](void* d, void* d_out) { return reduce_return_map_dev(m, d, n, d_out, nullptr); });
}

// ---- HEALPix point source and the fate map of its sky (kr_healpix.hip) ---------------------------------------------------------------------
int64_t kr_healpix_count(const kr_healpix_source* s, int64_t* npix)
{
    const int rc = healpix_validate(s, "kr_healpix_count");
    if (rc != KR_OK) return rc;
    const int64_t np = 12LL << (2 * s->order);
    if (npix) *npix = np;
    return s->rays_per_pixel * np;
}

int kr_healpix_vectors_dev_f64(int32_t order, int32_t unit_center, int64_t first_pix, int64_t stride, int64_t count, void* d_out, void* st)
{
    const int rc = healpix_vectors_validate(order, first_pix, stride, count, "kr_healpix_vectors");
    if (rc != KR_OK) return rc;
    return on_device(count == 0 || d_out, "kr_healpix_vectors: null output buffer",
                     [&] { return healpix_vectors_dev(order, unit_center, first_pix, stride, count, d_out, (hipStream_t) st); });
}

int kr_healpix_init_dev_f64(const kr_healpix_source* s, int64_t first, int64_t stride, void* d, int64_t count, void* st)
{
    const int rc = healpix_shard_validate(s, first, stride, count, "kr_healpix_init");
    if (rc != KR_OK) return rc;
    return on_device(count == 0 || d, "kr_healpix_init: null ray buffer", [&] { return healpix_init_dev(s, d, count, first, stride, false, 0, (hipStream_t) st); });
}

int kr_healpix_init_emit_dev_f64(const kr_healpix_source* s, int64_t first, int64_t stride, int reverse, void* d, int64_t count, void* st)
{
    const int rc = healpix_shard_validate(s, first, stride, count, "kr_healpix_init_emit");
    if (rc != KR_OK) return rc;
    return on_device(count == 0 || d, "kr_healpix_init_emit: null ray buffer",
                     [&] { return healpix_init_dev(s, d, count, first, stride, true, reverse, (hipStream_t) st); });
}

int kr_healpix_init_f64(const kr_healpix_source* s, kr_ray_f64* rays, int64_t n)
{
    const int rc = healpix_validate(s, "kr_healpix_init");
    if (rc != KR_OK) return rc;
    if (n != kr_healpix_count(s, nullptr)) return invalid("kr_healpix_init: n is not kr_healpix_count()");
    return with_staged_rays(rays, n, sizeof(kr_ray_f64), kConstructs, nullptr, [&](void* d) { return healpix_init_dev(s, d, n, 0, 1, false, 0, nullptr); });
}

int kr_post_healpix_map_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_healpix_map* m, void* d, int64_t n,
                                int64_t first, int64_t stride, void* d_out, void* st)
{
    int rc = refuse_plunge(V, "kr_post_healpix_map");
    if (rc == KR_OK) rc = healpix_map_validate(m, n, first, stride, "kr_post_healpix_map");
    if (rc != KR_OK) return rc;
    return on_device(d_out && (n == 0 || d), "kr_post_healpix_map: null argument",
                     [&] { return post_healpix_map_dev(spin, V, reverse, projradius, motion, lo, hi, m, d, n, first, stride, d_out, (hipStream_t) st); });
}

int kr_reduce_healpix_map_dev_f64(const kr_healpix_map* m, const void* d, int64_t n, int64_t first, int64_t stride, void* d_out, void* st)
{
    const int rc = healpix_map_validate(m, n, first, stride, "kr_reduce_healpix_map");
    if (rc != KR_OK) return rc;
    return on_device(d_out && (n == 0 || d), "kr_reduce_healpix_map: null argument",
                     [&] { return reduce_healpix_map_dev(m, d, n, first, stride, d_out, (hipStream_t) st); });
}

int kr_reduce_healpix_map_f64(const kr_healpix_map* m, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = healpix_map_validate(m, n, 0, 1, "kr_reduce_healpix_map");
    if (rc != KR_OK) return rc;
    if (!out) return invalid("kr_reduce_healpix_map: null argument");
    return reduce_to_host(rays, n, 7 * (size_t) m->npix + 6, out, [&](void* d, void* d_out) { return reduce_healpix_map_dev(m, d, n, 0, 1, d_out, nullptr); });
}

// ---- point source with any four-velocity (kr_source_vel.hip) and the angular distribution of where its rays end (kr_angdist.hip) ------------
int64_t kr_pointsource_vel_count(const kr_pointsource_vel_spec* s, int32_t* n_cosalpha, int32_t* n_beta)
{
    int64_t total;
    int nc, nb;
    if (!s || !pointsource_vel_grid(s, &total, &nc, &nb)) { set_error("kr_pointsource_vel_count: null spec or a grid whose ray count is not a non-negative int"); return -1; }
    if (n_cosalpha) *n_cosalpha = nc;
    if (n_beta) *n_beta = nb;
    return total;
}

int kr_pointsource_vel_tetrad(const kr_pointsource_vel_spec* s, double* tetrad16)
{
    krvel::Frame f;
    const int rc = pointsource_vel_validate(s, "kr_pointsource_vel_tetrad", &f);
    if (rc != KR_OK) return rc;
    if (!tetrad16) return invalid("kr_pointsource_vel_tetrad: null argument");
    std::memcpy(tetrad16, f.tetrad, sizeof f.tetrad);
    return KR_OK;
}

// the checks every init form makes, in the header's order; *f: the emitter's frame of a spec that passed
static int pointsource_vel_check(const kr_pointsource_vel_spec* s, const void* rays, int64_t n, const char* who, krvel::Frame* f)
{
    if (!s) return invalid_arg(who, "null spec");
    if (n < 0) return invalid_arg(who, "negative n");
    if (n > 0 && !rays) return invalid_arg(who, "null ray buffer");
    const int rc = pointsource_vel_validate(s, who, f);
    if (rc != KR_OK) return rc;
    if (n != kr_pointsource_vel_count(s, nullptr, nullptr)) return invalid_arg(who, "n is not kr_pointsource_vel_count()");
    return KR_OK;
}

int kr_pointsource_vel_init_dev_f64(const kr_pointsource_vel_spec* s, void* d, int64_t n, void* st)
{
    krvel::Frame f;
    const int rc = pointsource_vel_check(s, d, n, "kr_pointsource_vel_init", &f);
    if (rc != KR_OK) return rc;
    return on_device(true, nullptr, [&] { return pointsource_vel_init_dev(s, &f, d, n, false, (hipStream_t) st); });
}

int kr_pointsource_vel_init_emit_dev_f64(const kr_pointsource_vel_spec* s, void* d, int64_t n, void* st)
{
    krvel::Frame f;
    const int rc = pointsource_vel_check(s, d, n, "kr_pointsource_vel_init_emit", &f);
    if (rc != KR_OK) return rc;
    return on_device(true, nullptr, [&] { return pointsource_vel_init_dev(s, &f, d, n, true, (hipStream_t) st); });
}

int kr_pointsource_vel_init_f64(const kr_pointsource_vel_spec* s, kr_ray_f64* rays, int64_t n)
{
    krvel::Frame f;
    const int rc = pointsource_vel_check(s, rays, n, "kr_pointsource_vel_init", &f);
    if (rc != KR_OK) return rc;
    return with_staged_rays(rays, n, sizeof(kr_ray_f64), kConstructs, nullptr, [&](void* d) { return pointsource_vel_init_dev(s, &f, d, n, false, nullptr); });
}

int kr_angdist_nangle(const kr_angdist_spec* sp)
{
    return angdist_validate(sp, "kr_angdist_nangle") == KR_OK ? angdist_nangle(sp) : -1;
}

int kr_reduce_angdist_dev_f64(const kr_angdist_spec* sp, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = angdist_validate(sp, "kr_reduce_angdist");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_angdist: null argument or negative n", [&] { return reduce_angdist_dev(sp, d, n, d_out, (hipStream_t) st); });
}

int kr_post_angdist_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_angdist_spec* sp, void* d, int64_t n,
                            void* d_out, void* st)
{
    int rc = refuse_plunge(V, "kr_post_angdist");
    if (rc == KR_OK) rc = angdist_validate(sp, "kr_post_angdist");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_angdist: null argument or negative n",
                     [&] { return post_angdist_dev(spin, V, reverse, projradius, motion, lo, hi, sp, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_angdist_f64(const kr_angdist_spec* sp, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = angdist_validate(sp, "kr_reduce_angdist");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_angdist: null argument or negative n");
    return reduce_to_host(rays, n, 14 * (size_t) angdist_nangle(sp) + 8, out, [&](void* d, void* d_out) { return reduce_angdist_dev(sp, d, n, d_out, nullptr); });
}

// ---- the source-to-observer link (kr_observer.hip) ---------------------------------------------------------------------------------------------
int kr_reduce_observer_dev_f64(const kr_observer_spec* sp, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = observer_validate(sp, "kr_reduce_observer");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_observer: null argument or negative n", [&] { return reduce_observer_dev(sp, d, n, d_out, (hipStream_t) st); });
}

int kr_post_observer_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_observer_spec* sp, void* d, int64_t n,
                             void* d_out, void* st)
{
    int rc = refuse_plunge(V, "kr_post_observer");
    if (rc == KR_OK) rc = observer_validate(sp, "kr_post_observer");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_observer: null argument or negative n",
                     [&] { return post_observer_dev(spin, V, reverse, projradius, motion, lo, hi, sp, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_observer_f64(const kr_observer_spec* sp, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = observer_validate(sp, "kr_reduce_observer");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_observer: null argument or negative n");
    return reduce_to_host(rays, n, (size_t) observer_words(sp), out, [&](void* d, void* d_out) { return reduce_observer_dev(sp, d, n, d_out, nullptr); });
}

// ---- the (r, phi) illumination map (kr_illum.hip) --------------------------------------------------------------------------------------------------
int kr_reduce_illum_dev_f64(const kr_illum_bins* m, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = illum_validate(m, "kr_reduce_illum");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_illum: null argument or negative n", [&] { return reduce_illum_dev(m, d, n, d_out, (hipStream_t) st); });
}

int kr_post_illum_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_illum_bins* m, void* d, int64_t n, void* d_out,
                          void* st)
{
    int rc = refuse_plunge(V, "kr_post_illum");
    if (rc == KR_OK) rc = illum_validate(m, "kr_post_illum");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_illum: null argument or negative n",
                     [&] { return post_illum_dev(spin, V, reverse, projradius, motion, lo, hi, m, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_illum_f64(const kr_illum_bins* m, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = illum_validate(m, "kr_reduce_illum");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_illum: null argument or negative n");
    return reduce_to_host(rays, n, (size_t) illum_words(m), out, [&](void* d, void* d_out) { return reduce_illum_dev(m, d, n, d_out, nullptr); });
}

int kr_reduce_line_dev_f64(const kr_line_bins* b, const void* d, int64_t n, void* d_line, void* st)
{
    const int rc = line_validate(b, "kr_reduce_line");
    if (rc != KR_OK) return rc;
    return on_device(d_line && (n <= 0 || d), "kr_reduce_line: null argument", [&] { return reduce_line_dev(b, d, n, d_line, (hipStream_t) st); });
}

int kr_post_line_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_line_bins* b, void* d, int64_t n,
                         void* d_line, void* st)
{
    int rc = accept_plunge(V, motion, "kr_post_line");
    if (rc == KR_OK) rc = line_validate(b, "kr_post_line");
    if (rc != KR_OK) return rc;
    return on_device(d_line && (n <= 0 || d), "kr_post_line: null argument",
                     [&] { return post_line_dev(spin, V, reverse, projradius, motion, lo, hi, b, d, n, d_line, (hipStream_t) st); });
}

int kr_line_from_image_dev_f64(const kr_line_bins* b, const kr_image_bins* ib, const void* d_planes, void* d_line, void* st)
{
    const int rc = line_validate(b, "kr_line_from_image");
    if (rc != KR_OK) return rc;
    if (!ib || !d_planes || !d_line) return invalid("kr_line_from_image: null argument");
    return on_device(ib->img_nx > 0 && ib->img_ny > 0, "kr_line_from_image: image size must be positive",
                     [&] { return line_from_image_dev(b, ib, d_planes, d_line, (hipStream_t) st); });
}

int kr_reduce_line_f64(const kr_line_bins* b, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = line_validate(b, "kr_reduce_line");
    if (rc != KR_OK) return rc;
    if (!out || (n > 0 && !rays)) return invalid("kr_reduce_line: null argument");
    std::vector<double> h((size_t) 2 * b->nt * b->ne + 2, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_line) { return reduce_line_dev(b, d, n, d_line, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, h.data(), h.size() * sizeof(double));
    return rc2;
}

// ---- photon angles in the disc frame (kr_angles.hip; the limb-darkened line: kr_line.hip): everything is validated before anything touches a device ----
int kr_angles_dev_f64(double spin, double V, int reverse, int projradius, int motion, const void* d, int64_t n, void* d_angles, void* st)
{
    const int rc = angles_validate(motion, "kr_angles");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && (n == 0 || (d && d_angles)), "kr_angles: null argument or negative n",
                     [&] { return angles_dev(spin, V, reverse, projradius, d, n, d_angles, (hipStream_t) st); });
}

int kr_angles_f64(double spin, double V, int reverse, int projradius, int motion, const kr_ray_f64* rays, int64_t n, double* angles)
{
    const int rc = angles_validate(motion, "kr_angles");
    if (rc != KR_OK) return rc;
    if (n < 0 || (n > 0 && (!rays || !angles))) return invalid("kr_angles: null argument or negative n");
    return with_staged_rays((void*) rays, n, sizeof(kr_ray_f64), kReads, nullptr, [&](void* d) -> int {
        if (n == 0) return KR_OK;
        DeviceBuffer d_angles;
        int rc2 = d_angles.alloc((size_t) n * 2 * sizeof(double));
        if (rc2 != KR_OK) return rc2;
        rc2 = angles_dev(spin, V, reverse, projradius, d, n, d_angles.p, nullptr);
        if (rc2 != KR_OK) return rc2;
        KR_HIP(hipMemcpy(angles, d_angles.p, (size_t) n * 2 * sizeof(double), hipMemcpyDeviceToHost));
        return (int) KR_OK;
    });
}

int kr_post_line_limb_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law,
                              void* d, int64_t n, void* d_line, void* st)
{
    int rc = line_validate(b, "kr_post_line_limb");
    if (rc == KR_OK) rc = limb_validate(law, "kr_post_line_limb");
    if (rc == KR_OK) rc = angles_validate(motion, "kr_post_line_limb");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_line && (n == 0 || d), "kr_post_line_limb: null argument or negative n",
                     [&] { return post_line_limb_dev(spin, V, reverse, projradius, lo, hi, b, law, d, n, d_line, (hipStream_t) st); });
}

int kr_post_emissivity_mu_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_emis_bins* b, const kr_mu_bins* mb,
                                  void* d, int64_t n, void* d_hist, void* d_mu, void* st)
{
    int rc = emissivity_mu_validate(b, mb, "kr_post_emissivity_mu");
    if (rc == KR_OK) rc = angles_validate(motion, "kr_post_emissivity_mu");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_hist && d_mu && (n == 0 || d), "kr_post_emissivity_mu: null argument or negative n",
                     [&] { return post_emissivity_mu_dev(spin, V, reverse, projradius, lo, hi, b, mb, d, n, d_hist, d_mu, (hipStream_t) st); });
}

// ---- continuum spectrum of the disc (kr_spectrum.hip): everything is validated before anything touches a device ----
int kr_post_spectrum_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_spectrum_model* m, const kr_limb_law* law,
                             void* d, int64_t n, void* d_out, void* st)
{
    int rc = accept_plunge(V, motion, "kr_post_spectrum");
    if (rc == KR_OK) rc = spectrum_validate(m, "kr_post_spectrum");
    if (rc == KR_OK) rc = spectrum_law_validate(law, motion, "kr_post_spectrum");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_spectrum: null argument or negative n",
                     [&] { return post_spectrum_dev(spin, V, reverse, projradius, motion, lo, hi, m, law, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_spectrum_dev_f64(const kr_spectrum_model* m, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = spectrum_validate(m, "kr_reduce_spectrum");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_spectrum: null argument or negative n", [&] { return reduce_spectrum_dev(m, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_spectrum_f64(const kr_spectrum_model* m, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = spectrum_validate(m, "kr_reduce_spectrum");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_spectrum: null argument or negative n");
    std::vector<double> h((size_t) m->ne + 4, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_out) { return reduce_spectrum_dev(m, d, n, d_out, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, h.data(), h.size() * sizeof(double));
    return rc2;
}

// ---- reverberation response of the disc (kr_response.hip): everything is validated before anything touches a device ----
int kr_post_response_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r, const kr_limb_law* law,
                             void* d, int64_t n, void* d_out, void* st)
{
    int rc = accept_plunge(V, motion, "kr_post_response");
    if (rc == KR_OK) rc = response_validate(r, "kr_post_response");
    if (rc == KR_OK) rc = spectrum_law_validate(law, motion, "kr_post_response");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_response: null argument or negative n",
                     [&] { return post_response_dev(spin, V, reverse, projradius, motion, lo, hi, r, law, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_response_dev_f64(const kr_response_model* r, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = response_validate(r, "kr_reduce_response");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_response: null argument or negative n", [&] { return reduce_response_dev(r, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_response_f64(const kr_response_model* r, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = response_validate(r, "kr_reduce_response");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_response: null argument or negative n");
    std::vector<double> h((size_t) r->nt * r->spec.ne + 4, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_out) { return reduce_response_dev(r, d, n, d_out, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, h.data(), h.size() * sizeof(double));
    return rc2;
}

// ---- the line and the response driven by an (r, phi) illumination table (kr_illum_table; the ILLUM flavour of kr_line.hip and kr_response.hip): what the
//      flat twin validates, then the table, then that the bins / the model carry no radial table of their own; nothing touches a device before that ----
namespace {
int line_illum_validate(const kr_line_bins* b, const kr_illum_table* t, const char* who)
{
    int rc = line_validate(b, who);
    if (rc == KR_OK) rc = illum_table_validate(t, who);
    if (rc == KR_OK && (b->table_emis || b->table_time)) rc = invalid_arg(who, "the bins carry a radial table as well as the (r, phi) table");
    return rc;
}
int response_illum_validate(const kr_response_model* r, const kr_illum_table* t, const char* who)
{
    int rc = response_validate(r, who);
    if (rc == KR_OK) rc = illum_table_validate(t, who);
    if (rc == KR_OK && (r->spec.table_emis || r->table_time)) rc = invalid_arg(who, "the model carries a radial table as well as the (r, phi) table");
    return rc;
}
}  // namespace

int kr_post_line_illum_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law,
                               const kr_illum_table* t, void* d, int64_t n, void* d_line, void* st)
{
    int rc = refuse_plunge(V, "kr_post_line_illum");
    if (rc == KR_OK) rc = line_illum_validate(b, t, "kr_post_line_illum");
    if (rc == KR_OK) rc = limb_validate(law, "kr_post_line_illum");
    if (rc == KR_OK) rc = angles_validate(motion, "kr_post_line_illum");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_line && (n == 0 || d), "kr_post_line_illum: null argument or negative n",
                     [&] { return post_line_illum_dev(spin, V, reverse, projradius, lo, hi, b, law, t, d, n, d_line, (hipStream_t) st); });
}

int kr_reduce_line_illum_dev_f64(const kr_line_bins* b, const kr_illum_table* t, const void* d, int64_t n, void* d_line, void* st)
{
    const int rc = line_illum_validate(b, t, "kr_reduce_line_illum");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_line && (n == 0 || d), "kr_reduce_line_illum: null argument or negative n",
                     [&] { return reduce_line_illum_dev(b, t, d, n, d_line, (hipStream_t) st); });
}

int kr_reduce_line_illum_f64(const kr_line_bins* b, const kr_illum_table* t, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = line_illum_validate(b, t, "kr_reduce_line_illum");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_line_illum: null argument or negative n");
    std::vector<double> h((size_t) 2 * b->nt * b->ne + 2, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_line) { return reduce_line_illum_dev(b, t, d, n, d_line, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, h.data(), h.size() * sizeof(double));
    return rc2;
}

int kr_post_response_illum_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r,
                                   const kr_limb_law* law, const kr_illum_table* t, void* d, int64_t n, void* d_out, void* st)
{
    int rc = refuse_plunge(V, "kr_post_response_illum");
    if (rc == KR_OK) rc = response_illum_validate(r, t, "kr_post_response_illum");
    if (rc == KR_OK) rc = spectrum_law_validate(law, motion, "kr_post_response_illum");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_response_illum: null argument or negative n",
                     [&] { return post_response_illum_dev(spin, V, reverse, projradius, motion, lo, hi, r, law, t, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_response_illum_dev_f64(const kr_response_model* r, const kr_illum_table* t, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = response_illum_validate(r, t, "kr_reduce_response_illum");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_response_illum: null argument or negative n",
                     [&] { return reduce_response_illum_dev(r, t, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_response_illum_f64(const kr_response_model* r, const kr_illum_table* t, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = response_illum_validate(r, t, "kr_reduce_response_illum");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_response_illum: null argument or negative n");
    std::vector<double> h((size_t) r->nt * r->spec.ne + 4, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_out) { return reduce_response_illum_dev(r, t, d, n, d_out, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, h.data(), h.size() * sizeof(double));
    return rc2;
}

// ---- the passes over rays that landed on a disc surface (kr_disc_surface; the SURFACE flavour of kr_line.hip, kr_spectrum.hip, kr_response.hip and the
//      per-record angles of kr_angles.hip): the surface first, then what the flat twin validates; nothing touches a device before that ----
int kr_angles_surface_dev_f64(const kr_disc_surface* s, double spin, int reverse, const void* d, int64_t n, void* d_angles, void* st)
{
    const int rc = surface_validate(s, "kr_angles_surface");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && (n == 0 || (d && d_angles)), "kr_angles_surface: null argument or negative n",
                     [&] { return angles_surface_dev(s, spin, reverse, d, n, d_angles, (hipStream_t) st); });
}

int kr_angles_surface_f64(const kr_disc_surface* s, double spin, int reverse, const kr_ray_f64* rays, int64_t n, double* angles)
{
    const int rc = surface_validate(s, "kr_angles_surface");
    if (rc != KR_OK) return rc;
    if (n < 0 || (n > 0 && (!rays || !angles))) return invalid("kr_angles_surface: null argument or negative n");
    return with_staged_rays((void*) rays, n, sizeof(kr_ray_f64), kReads, nullptr, [&](void* d) -> int {
        if (n == 0) return KR_OK;
        DeviceBuffer d_angles;
        int rc2 = d_angles.alloc((size_t) n * 2 * sizeof(double));
        if (rc2 != KR_OK) return rc2;
        rc2 = angles_surface_dev(s, spin, reverse, d, n, d_angles.p, nullptr);
        if (rc2 != KR_OK) return rc2;
        KR_HIP(hipMemcpy(angles, d_angles.p, (size_t) n * 2 * sizeof(double), hipMemcpyDeviceToHost));
        return (int) KR_OK;
    });
}

int kr_post_line_surface_dev_f64(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law, void* d, int64_t n,
                                 void* d_line, void* st)
{
    int rc = surface_validate(s, "kr_post_line_surface");
    if (rc == KR_OK) rc = line_validate(b, "kr_post_line_surface");
    if (rc == KR_OK) rc = limb_validate(law, "kr_post_line_surface");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_line && (n == 0 || d), "kr_post_line_surface: null argument or negative n",
                     [&] { return post_line_surface_dev(s, spin, reverse, lo, hi, b, law, d, n, d_line, (hipStream_t) st); });
}

int kr_reduce_line_surface_dev_f64(const kr_disc_surface* s, const kr_line_bins* b, const void* d, int64_t n, void* d_line, void* st)
{
    int rc = surface_validate(s, "kr_reduce_line_surface");
    if (rc == KR_OK) rc = line_validate(b, "kr_reduce_line_surface");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_line && (n == 0 || d), "kr_reduce_line_surface: null argument or negative n",
                     [&] { return reduce_line_surface_dev(b, d, n, d_line, (hipStream_t) st); });
}

int kr_post_spectrum_surface_dev_f64(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_spectrum_model* m, const kr_limb_law* law, void* d,
                                     int64_t n, void* d_out, void* st)
{
    int rc = surface_validate(s, "kr_post_spectrum_surface");
    if (rc == KR_OK) rc = spectrum_validate(m, "kr_post_spectrum_surface");
    if (rc == KR_OK) rc = limb_validate(law, "kr_post_spectrum_surface");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_spectrum_surface: null argument or negative n",
                     [&] { return post_spectrum_surface_dev(s, spin, reverse, lo, hi, m, law, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_spectrum_surface_dev_f64(const kr_disc_surface* s, const kr_spectrum_model* m, const void* d, int64_t n, void* d_out, void* st)
{
    int rc = surface_validate(s, "kr_reduce_spectrum_surface");
    if (rc == KR_OK) rc = spectrum_validate(m, "kr_reduce_spectrum_surface");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_spectrum_surface: null argument or negative n",
                     [&] { return reduce_spectrum_surface_dev(m, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_spectrum_surface_f64(const kr_disc_surface* s, const kr_spectrum_model* m, const kr_ray_f64* rays, int64_t n, double* out)
{
    int rc = surface_validate(s, "kr_reduce_spectrum_surface");
    if (rc == KR_OK) rc = spectrum_validate(m, "kr_reduce_spectrum_surface");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_spectrum_surface: null argument or negative n");
    std::vector<double> h((size_t) m->ne + 4, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_out) { return reduce_spectrum_surface_dev(m, d, n, d_out, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, h.data(), h.size() * sizeof(double));
    return rc2;
}

int kr_post_response_surface_dev_f64(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_response_model* r, const kr_limb_law* law, void* d,
                                     int64_t n, void* d_out, void* st)
{
    int rc = surface_validate(s, "kr_post_response_surface");
    if (rc == KR_OK) rc = response_validate(r, "kr_post_response_surface");
    if (rc == KR_OK) rc = limb_validate(law, "kr_post_response_surface");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_response_surface: null argument or negative n",
                     [&] { return post_response_surface_dev(s, spin, reverse, lo, hi, r, law, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_response_surface_dev_f64(const kr_disc_surface* s, const kr_response_model* r, const void* d, int64_t n, void* d_out, void* st)
{
    int rc = surface_validate(s, "kr_reduce_response_surface");
    if (rc == KR_OK) rc = response_validate(r, "kr_reduce_response_surface");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_response_surface: null argument or negative n",
                     [&] { return reduce_response_surface_dev(r, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_response_surface_f64(const kr_disc_surface* s, const kr_response_model* r, const kr_ray_f64* rays, int64_t n, double* out)
{
    int rc = surface_validate(s, "kr_reduce_response_surface");
    if (rc == KR_OK) rc = response_validate(r, "kr_reduce_response_surface");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_response_surface: null argument or negative n");
    std::vector<double> h((size_t) r->nt * r->spec.ne + 4, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, h.size(), h.data(), [&](void* d, void* d_out) { return reduce_response_surface_dev(r, d, n, d_out, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, h.data(), h.size() * sizeof(double));
    return rc2;
}

// ---- orbiting hot spot (kr_hotspot.hip): everything is validated before anything touches a device ----
int kr_post_hotspot_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_hotspot* h, const kr_limb_law* law, void* d,
                            int64_t n, void* d_out, void* st)
{
    int rc = refuse_plunge(V, "kr_post_hotspot");
    if (rc == KR_OK) rc = hotspot_validate(h, "kr_post_hotspot");
    if (rc == KR_OK) rc = spectrum_law_validate(law, motion, "kr_post_hotspot");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_hotspot: null argument or negative n",
                     [&] { return post_hotspot_dev(spin, V, reverse, projradius, motion, lo, hi, h, law, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_hotspot_dev_f64(const kr_hotspot* h, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = hotspot_validate(h, "kr_reduce_hotspot");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_hotspot: null argument or negative n", [&] { return reduce_hotspot_dev(h, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_hotspot_f64(const kr_hotspot* h, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = hotspot_validate(h, "kr_reduce_hotspot");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_hotspot: null argument or negative n");
    std::vector<double> w((size_t) h->nt * (3 + (size_t) h->ne) + 4, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, w.size(), w.data(), [&](void* d, void* d_out) { return reduce_hotspot_dev(h, d, n, d_out, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, w.data(), w.size() * sizeof(double));
    return rc2;
}

// the Stokes spectra of the continuum: the refusals of the model, of the polarisation entry points and of the two laws, in that order
static int spectrum_stokes_validate(double V, int reverse, int motion, double inc_deg, const kr_spectrum_model* m, const kr_limb_law* law, const kr_pol_law* pol, const char* who)
{
    int rc = refuse_plunge(V, who);
    if (rc == KR_OK) rc = spectrum_validate(m, who);
    if (rc == KR_OK) rc = polarisation_validate(reverse, motion, inc_deg, who);
    if (rc == KR_OK) rc = limb_validate(law, who);
    if (rc == KR_OK) rc = pol_validate(pol, who);
    return rc;
}

int kr_post_spectrum_stokes_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, double inc_deg, const kr_spectrum_model* m,
                                    const kr_limb_law* law, const kr_pol_law* pol, void* d, int64_t n, void* d_out, void* st)
{
    const int rc = spectrum_stokes_validate(V, reverse, motion, inc_deg, m, law, pol, "kr_post_spectrum_stokes");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_spectrum_stokes: null argument or negative n",
                     [&] { return post_spectrum_stokes_dev(spin, V, reverse, projradius, lo, hi, inc_deg, m, law, pol, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_spectrum_stokes_dev_f64(double spin, double V, int reverse, int projradius, double inc_deg, const kr_spectrum_model* m, const kr_limb_law* law,
                                      const kr_pol_law* pol, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = spectrum_stokes_validate(V, reverse, 0, inc_deg, m, law, pol, "kr_reduce_spectrum_stokes");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_spectrum_stokes: null argument or negative n",
                     [&] { return reduce_spectrum_stokes_dev(spin, V, reverse, projradius, inc_deg, m, law, pol, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_spectrum_stokes_f64(double spin, double V, int reverse, int projradius, double inc_deg, const kr_spectrum_model* m, const kr_limb_law* law,
                                  const kr_pol_law* pol, const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = spectrum_stokes_validate(V, reverse, 0, inc_deg, m, law, pol, "kr_reduce_spectrum_stokes");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_spectrum_stokes: null argument or negative n");
    std::vector<double> w(3 * (size_t) m->ne + 4, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, w.size(), w.data(),
                                   [&](void* d, void* d_out) { return reduce_spectrum_stokes_dev(spin, V, reverse, projradius, inc_deg, m, law, pol, d, n, d_out, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, w.data(), w.size() * sizeof(double));
    return rc2;
}

// the Stokes light curves of the spot: the refusals of the spot, of the polarisation entry points and of the two laws, in that order
static int hotspot_stokes_validate(double V, int reverse, int motion, double inc_deg, const kr_hotspot* h, const kr_limb_law* law, const kr_pol_law* pol, const char* who)
{
    int rc = refuse_plunge(V, who);
    if (rc == KR_OK) rc = hotspot_validate(h, who);
    if (rc == KR_OK) rc = polarisation_validate(reverse, motion, inc_deg, who);
    if (rc == KR_OK) rc = limb_validate(law, who);
    if (rc == KR_OK) rc = pol_validate(pol, who);
    return rc;
}

int kr_post_hotspot_stokes_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, double inc_deg, const kr_hotspot* h,
                                   const kr_limb_law* law, const kr_pol_law* pol, void* d, int64_t n, void* d_out, void* st)
{
    const int rc = hotspot_stokes_validate(V, reverse, motion, inc_deg, h, law, pol, "kr_post_hotspot_stokes");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_hotspot_stokes: null argument or negative n",
                     [&] { return post_hotspot_stokes_dev(spin, V, reverse, projradius, lo, hi, inc_deg, h, law, pol, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_hotspot_stokes_dev_f64(double spin, double V, int reverse, int projradius, double inc_deg, const kr_hotspot* h, const kr_limb_law* law,
                                     const kr_pol_law* pol, const void* d, int64_t n, void* d_out, void* st)
{
    const int rc = hotspot_stokes_validate(V, reverse, 0, inc_deg, h, law, pol, "kr_reduce_hotspot_stokes");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_reduce_hotspot_stokes: null argument or negative n",
                     [&] { return reduce_hotspot_stokes_dev(spin, V, reverse, projradius, inc_deg, h, law, pol, d, n, d_out, (hipStream_t) st); });
}

int kr_reduce_hotspot_stokes_f64(double spin, double V, int reverse, int projradius, double inc_deg, const kr_hotspot* h, const kr_limb_law* law, const kr_pol_law* pol,
                                 const kr_ray_f64* rays, int64_t n, double* out)
{
    const int rc = hotspot_stokes_validate(V, reverse, 0, inc_deg, h, law, pol, "kr_reduce_hotspot_stokes");
    if (rc != KR_OK) return rc;
    if (!out || n < 0 || (n > 0 && !rays)) return invalid("kr_reduce_hotspot_stokes: null argument or negative n");
    std::vector<double> w((size_t) h->nt * (5 + (size_t) h->ne) + 4, 0.0);        // out is written only by a call that succeeds
    const int rc2 = reduce_to_host(rays, n, w.size(), w.data(),
                                   [&](void* d, void* d_out) { return reduce_hotspot_stokes_dev(spin, V, reverse, projradius, inc_deg, h, law, pol, d, n, d_out, nullptr); });
    if (rc2 == KR_OK) std::memcpy(out, w.data(), w.size() * sizeof(double));
    return rc2;
}

// ---- polarisation of disc emission (kr_polarisation.hip; the Stokes line: kr_line.hip): everything is validated before anything touches a device ----
int kr_polarisation_dev_f64(double spin, double V, int reverse, int projradius, int motion, double inc_deg, const void* d, int64_t n, void* d_out, void* st)
{
    int rc = refuse_plunge(V, "kr_polarisation");
    if (rc == KR_OK) rc = polarisation_validate(reverse, motion, inc_deg, "kr_polarisation");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && (n == 0 || (d && d_out)), "kr_polarisation: null argument or negative n",
                     [&] { return polarisation_dev(spin, V, reverse, projradius, inc_deg, d, n, d_out, (hipStream_t) st); });
}

int kr_polarisation_f64(double spin, double V, int reverse, int projradius, int motion, double inc_deg, const kr_ray_f64* rays, int64_t n, double* out)
{
    int rc = refuse_plunge(V, "kr_polarisation");
    if (rc == KR_OK) rc = polarisation_validate(reverse, motion, inc_deg, "kr_polarisation");
    if (rc != KR_OK) return rc;
    if (n < 0 || (n > 0 && (!rays || !out))) return invalid("kr_polarisation: null argument or negative n");
    return with_staged_rays((void*) rays, n, sizeof(kr_ray_f64), kReads, nullptr, [&](void* d) -> int {
        if (n == 0) return KR_OK;
        DeviceBuffer d_out;
        int rc2 = d_out.alloc((size_t) n * 4 * sizeof(double));
        if (rc2 != KR_OK) return rc2;
        rc2 = polarisation_dev(spin, V, reverse, projradius, inc_deg, d, n, d_out.p, nullptr);
        if (rc2 != KR_OK) return rc2;
        KR_HIP(hipMemcpy(out, d_out.p, (size_t) n * 4 * sizeof(double), hipMemcpyDeviceToHost));
        return (int) KR_OK;
    });
}

int kr_post_image_stokes_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, double inc_deg, const kr_image_bins* b,
                                 const kr_limb_law* limb, const kr_pol_law* pol, void* d, int64_t n, void* d_stokes, void* st)
{
    if (refuse_plunge(V, "kr_post_image_stokes")) return KR_EINVAL;
    if (!b) return invalid("kr_post_image_stokes: null bins");
    if (b->img_nx <= 0 || b->img_ny <= 0) return invalid("kr_post_image_stokes: image size must be positive");
    int rc = limb_validate(limb, "kr_post_image_stokes");
    if (rc == KR_OK) rc = pol_validate(pol, "kr_post_image_stokes");
    if (rc == KR_OK) rc = polarisation_validate(reverse, motion, inc_deg, "kr_post_image_stokes");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_stokes && (n == 0 || d), "kr_post_image_stokes: null argument or negative n",
                     [&] { return post_image_stokes_dev(spin, V, reverse, projradius, lo, hi, inc_deg, b, limb, pol, d, n, d_stokes, (hipStream_t) st); });
}

int kr_post_line_stokes_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, double inc_deg, const kr_line_bins* b,
                                const kr_limb_law* limb, const kr_pol_law* pol, void* d, int64_t n, void* d_out, void* st)
{
    int rc = refuse_plunge(V, "kr_post_line_stokes");
    if (rc == KR_OK) rc = line_validate(b, "kr_post_line_stokes");
    if (rc == KR_OK) rc = limb_validate(limb, "kr_post_line_stokes");
    if (rc == KR_OK) rc = pol_validate(pol, "kr_post_line_stokes");
    if (rc == KR_OK) rc = polarisation_validate(reverse, motion, inc_deg, "kr_post_line_stokes");
    if (rc != KR_OK) return rc;
    return on_device(n >= 0 && d_out && (n == 0 || d), "kr_post_line_stokes: null argument or negative n",
                     [&] { return post_line_stokes_dev(spin, V, reverse, projradius, lo, hi, inc_deg, b, limb, pol, d, n, d_out, (hipStream_t) st); });
}

// ---- critical-curve maps (kr_caustic.hip): everything is validated before anything touches a device --------------------------------------
int kr_bundles_init_emit_dev_f64(const kr_imageplane* s, double eps_frac, double V, int reverse, int projradius, void* d, int64_t n, void* st)
{
    if (!s) return invalid("kr_bundles_init_emit: null spec");
    if (refuse_plunge(V, "kr_bundles_init_emit")) return KR_EINVAL;
    if (!std::isfinite(eps_frac) || !(eps_frac > 0) || !(eps_frac < 0.5)) return invalid("kr_bundles_init_emit: eps_frac must lie in (0, 0.5)");
    int32_t nx = 0, ny = 0;
    kr_imageplane_count(s, &nx, &ny);
    if (nx < 1 || ny < 1) return invalid("kr_bundles_init_emit: empty ray grid (nx and ny must be >= 1)");
    if (n < 5 * (int64_t) nx * ny) return invalid("kr_bundles_init_emit: n smaller than 5 nx ny");
    return on_device(d, "kr_bundles_init_emit: null ray buffer",
                     [&] { return bundles_init_emit_dev(s, nx, ny, eps_frac, V, reverse, projradius, d, n, (hipStream_t) st); });
}

int kr_post_caustic_disc_dev_f64(double spin, int reverse, const kr_caustic_map* m, void* d, int64_t n, void* d_maps, void* st)
{
    const int rc = caustic_validate(m, n, "kr_post_caustic_disc");
    if (rc != KR_OK) return rc;
    return on_device(d && d_maps, "kr_post_caustic_disc: null argument", [&] { return post_caustic_dev(spin, reverse, m, d, n, d_maps, (hipStream_t) st); });
}

int kr_caustic_suppress_dev_f64(const kr_caustic_map* m, void* d_maps, void* st)
{
    const int rc = caustic_validate(m, INT64_MAX, "kr_caustic_suppress");       // no records here
    if (rc != KR_OK) return rc;
    return on_device(d_maps, "kr_caustic_suppress: null argument", [&] { return caustic_suppress_dev(m, d_maps, (hipStream_t) st); });
}

int kr_post_caustic_source_dev_f64(const kr_source_map* m, const void* d, int64_t n, void* d_maps, void* st)
{
    const int rc = source_map_validate(m, n, "kr_post_caustic_source");
    if (rc != KR_OK) return rc;
    return on_device(d && d_maps, "kr_post_caustic_source: null argument", [&] { return post_caustic_source_dev(m, d, d_maps, (hipStream_t) st); });
}

// ---- diagnostics ---------------------------------------------------------------------------------------------
int kr_debug_arith_f64(int op, const double* a, const double* b, double* out, int64_t n)
{
    if (!a || !b || !out || n < 0) return invalid("kr_debug_arith: bad argument");
    int rc = require_device();
    if (rc != KR_OK) return rc;
    if (n == 0) return KR_OK;
    DeviceBuffer da, db, dout;
    const size_t bytes = (size_t) n * sizeof(double);
    if ((rc = da.upload(a, bytes)) != KR_OK || (rc = db.upload(b, bytes)) != KR_OK || (rc = dout.alloc(bytes)) != KR_OK) return rc;
    rc = arith_probe_dev(op, (const double*) da.p, (const double*) db.p, (double*) dout.p, n);
    if (rc != KR_OK) return rc;
    KR_HIP(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    return KR_OK;
}

// ---- attached host arrays (see with_staged_rays) --------------------------------------------------------------------------
int kr_host_attach(void* rays, int64_t n, int32_t ray_bytes)
{
    if (!rays || n <= 0 || (ray_bytes != (int32_t) sizeof(kr_ray_f64) && ray_bytes != (int32_t) sizeof(kr_ray_f32))) return invalid("kr_host_attach: bad argument");
    int rc = require_device();
    if (rc != KR_OK) return rc;
    Attached a;
    a.host = rays; a.n = n; a.ray_bytes = (size_t) ray_bytes;
    {
        std::lock_guard<std::mutex> lk(g_att_mu);
        if (g_attached.count(rays)) return invalid("kr_host_attach: array is already attached");
    }
    hipError_t e = hipMalloc(&a.dev, (size_t) n * ray_bytes);
    if (e == hipSuccess) e = hipMalloc(&a.d_field, (size_t) n * 32);
    if (e == hipSuccess && !(a.h_field = std::malloc((size_t) n * 32))) e = hipErrorOutOfMemory;
    if (e != hipSuccess) { release_buffers(a); return hip_fail(e, "kr_host_attach allocation", __FILE__, __LINE__); }
    std::lock_guard<std::mutex> lk(g_att_mu);
    g_attached[rays] = a;
    return KR_OK;
}

int kr_host_detach(void* rays)
{
    Attached a;
    {
        std::lock_guard<std::mutex> lk(g_att_mu);
        auto it = g_attached.find(rays);
        if (it == g_attached.end()) return KR_OK;
        a = it->second;
        g_attached.erase(it);
    }
    release_buffers(a);
    (void) hipGetLastError();
    return KR_OK;
}

// ---- memory helpers ------------------------------------------------------------------------------------------
int kr_malloc(void** d_ptr, int64_t bytes)
{
    if (!d_ptr || bytes < 0) return invalid("kr_malloc: bad argument");
    int rc = require_device();
    if (rc != KR_OK) return rc;
    KR_HIP(hipMalloc(d_ptr, (size_t) (bytes ? bytes : 1)));
    return KR_OK;
}
int kr_free(void* d_ptr)
{
    KR_HIP(hipFree(d_ptr));
    return KR_OK;
}
int kr_host_alloc(void** h_ptr, int64_t bytes)
{
    if (!h_ptr || bytes < 0) return invalid("kr_host_alloc: bad argument");
    int rc = require_device();
    if (rc != KR_OK) return rc;
    KR_HIP(hipHostMalloc(h_ptr, (size_t) (bytes ? bytes : 1), hipHostMallocDefault));
    return KR_OK;
}
int kr_host_free(void* h_ptr)
{
    KR_HIP(hipHostFree(h_ptr));
    return KR_OK;
}
int kr_memcpy_h2d(void* d_dst, const void* h_src, int64_t bytes)
{
    KR_HIP(hipMemcpy(d_dst, h_src, (size_t) bytes, hipMemcpyHostToDevice));
    return KR_OK;
}
int kr_memcpy_d2h(void* h_dst, const void* d_src, int64_t bytes)
{
    KR_HIP(hipMemcpy(h_dst, d_src, (size_t) bytes, hipMemcpyDeviceToHost));
    return KR_OK;
}
int kr_memset(void* d_ptr, int value, int64_t bytes)
{
    KR_HIP(hipMemset(d_ptr, value, (size_t) bytes));
    return KR_OK;
}
int kr_synchronize(void* stream)
{
    KR_HIP(hipStreamSynchronize((hipStream_t) stream));
    return KR_OK;
}
int kr_stream_create(void** stream)
{
    if (!stream) return invalid("kr_stream_create: null argument");
    int rc = require_device();
    if (rc != KR_OK) return rc;
    hipStream_t s = nullptr;
    KR_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*) s;
    return KR_OK;
}
int kr_stream_destroy(void* stream)
{
    if (!stream) return KR_OK;
    KR_HIP(hipStreamSynchronize((hipStream_t) stream));
    side_stream_forget((hipStream_t) stream);
    KR_HIP(hipStreamDestroy((hipStream_t) stream));
    return KR_OK;
}
int kr_configure_process(void)
{
    if (g_runtime_touched) return 0;
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    return 1;
}
int kr_shutdown(void)
{
    if (!g_runtime_touched) return KR_OK;
    const int rc = trace_shutdown();       // (drains every device this library has used)
    if (rc != KR_OK) return rc;
    device_tables_shutdown();
    return KR_OK;
}

}  // extern "C"
