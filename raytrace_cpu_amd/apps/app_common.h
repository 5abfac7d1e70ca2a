// apps/app_common.h -- small helpers shared by the device-resident applications.
#ifndef KR_APP_COMMON_H_
#define KR_APP_COMMON_H_

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kr_trace.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"

namespace krapp {

inline void check(int rc, const char* what)
{
    if (rc != KR_OK) throw std::runtime_error(std::string(what) + ": " + kr_last_error());
}

// a program that creates its output file before its first device call asks first: exit 1 with the reason, no file
inline void require_device()
{
    if (kr_device_count() < 0) throw std::runtime_error(kr_last_error());
}

// A program's options: `--key=value` on the command line first, then `key = value` in the parameter file (--parfile, or the program's default
// file), then the default.  An error carries the text of ParameterArgs or ParameterFile, whichever was asked last.
class Options {
public:
    Options(int argc, char** argv, const std::string& default_parfile)
        : args(argc, argv), par(args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : default_parfile) {}

    bool on_command_line(const std::string& key) const { return args.key_exists("--" + key); }       // also a bare --key, such as --timing
    bool has(const std::string& key) const { return on_command_line(key) || par.key_exists(key); }
    double num(const std::string& key, double dflt) const { return get<double>(key, dflt); }
    double req(const std::string& key) const { return get<double>(key); }
    int integer(const std::string& key) const { return get<int>(key); }
    int integer(const std::string& key, int dflt) const { return get<int>(key, dflt); }
    bool flag(const std::string& key, bool dflt) const { return get<bool>(key, dflt); }               // 0 | 1
    std::string str(const std::string& key) const { return get<std::string>(key); }
    std::string str(const std::string& key, const std::string& dflt) const { return get<std::string>(key, dflt); }

    const ParameterArgs args;
    const ParameterFile par;

private:
    template <class T>
    T get(const std::string& key) const { return on_command_line(key) ? args.get_parameter<T>("--" + key) : par.get_parameter<T>(key); }
    template <class T>
    T get(const std::string& key, const T& dflt) const { return on_command_line(key) ? args.get_parameter<T>("--" + key) : par.get_parameter<T>(key, dflt); }
};

// main() of a program: the process set up for HIP, the options read, `body(options)`, "Done"; whatever is thrown goes to stderr with exit status 1
template <class Body>
inline int run_program(int argc, char** argv, const char* default_parfile, Body body)
try {
    (void) kr_configure_process();       // first HIP user of this process: hardware queues for overlapping launches (include/kr_trace.h)
    const Options opt(argc, argv, default_parfile);
    body(opt);
    std::cout << "Done" << std::endl;
    return 0;
} catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
}

// KRTRACE_ARITHMETIC = hybrid | strict | fast, as in the host mirror of the class API; unset: hybrid for the
// fixed-step integrators, strict for RK45
inline int arithmetic_flags(const std::string& choice, int integrator)
{
    if (choice.empty()) return integrator == KR_RK45 ? 0 : KR_FLAG_HYBRID;
    if (choice == "hybrid") return KR_FLAG_HYBRID;
    if (choice == "strict") return 0;
    if (choice == "fast") return KR_FLAG_FAST_MATH;
    throw std::invalid_argument("arithmetic: expected hybrid, strict or fast, got '" + choice + "'");
}
inline std::string arithmetic_from_env()
{
    const char* e = std::getenv("KRTRACE_ARITHMETIC");
    return e ? std::string(e) : std::string();
}
// --arithmetic, else the environment's (never the parameter file's)
inline std::string arithmetic_choice(const Options& opt)
{
    return opt.on_command_line("arithmetic") ? opt.str("arithmetic") : arithmetic_from_env();
}

// The disc flow keys of the programs that bin the disc (include/kr_trace.h, KR_V_PLUNGE): plunge = 0 | 1 and, read with plunge = 1 alone, r_in, the
// inner edge of what the program bins in place of the ISCO (default: 1.02 x the horizon radius).  plunge = 0: V = -1 and the ISCO, the program and
// its output files what they were.  With plunge = 1 a text file opens with the rows "# PLUNGE" and "# R_IN", a FITS header carries PLUNGE and R_IN.
struct DiscFlowKeys {
    bool plunge = false;
    double r_in = 0;
    double V() const { return plunge ? KR_V_PLUNGE : -1.0; }
    double inner_edge(double r_isco) const { return plunge ? r_in : r_isco; }
    template <class Text>
    void write_rows(Text& out) const
    {
        if (!plunge) return;
        out << "# PLUNGE" << 1 << std::endl;
        out << "# R_IN" << r_in << std::endl;
    }
    template <class Fits>
    void write_keywords(Fits& fits) const
    {
        if (!plunge) return;
        fits.write_keyword("PLUNGE", "Disc flow: Keplerian, plunging inside the ISCO", true);
        fits.write_keyword("R_IN", "Inner edge of what is binned", r_in);
    }
};

inline DiscFlowKeys disc_flow_keys(const Options& opt, double spin)
{
    DiscFlowKeys k;
    k.plunge = opt.flag("plunge", false);
    if (k.plunge) {
        const double horizon = kr_kerr_horizon(spin);
        k.r_in = opt.num("r_in", 1.02 * horizon);
        if (!(k.r_in > horizon)) throw std::invalid_argument("r_in: the inner edge must lie outside the horizon");
    }
    return k;
}

inline int integrator_code(const std::string& name, int fallback)
{
    if (name == "euler") return KR_EULER;
    if (name == "rk4") return KR_RK4;
    if (name == "rk45") return KR_RK45;
    return fallback;
}

// device buffer that frees itself
class DeviceBuffer {
public:
    explicit DeviceBuffer(int64_t bytes) : bytes_(bytes) { check(kr_malloc(&ptr_, bytes), "kr_malloc"); }
    ~DeviceBuffer() { if (ptr_) kr_free(ptr_); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    void* get() const { return ptr_; }
    void zero() { check(kr_memset(ptr_, 0, bytes_), "kr_memset"); }

private:
    void* ptr_ = nullptr;
    int64_t bytes_;
};

// page-locked host buffer of doubles (read-back target)
class PinnedDoubles {
public:
    explicit PinnedDoubles(int64_t count) : count_(count)
    {
        void* p = nullptr;
        check(kr_host_alloc(&p, count * (int64_t) sizeof(double)), "kr_host_alloc");
        ptr_ = static_cast<double*>(p);
    }
    ~PinnedDoubles() { if (ptr_) kr_host_free(ptr_); }
    PinnedDoubles(const PinnedDoubles&) = delete;
    PinnedDoubles& operator=(const PinnedDoubles&) = delete;
    double* data() const { return ptr_; }
    int64_t size() const { return count_; }
    double& operator[](int64_t i) const { return ptr_[i]; }

private:
    double* ptr_ = nullptr;
    int64_t count_;
};

class Stopwatch {
public:
    Stopwatch() : t0_(std::chrono::steady_clock::now()) {}
    double lap_ms()
    {
        const auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0_).count();
        t0_ = t1;
        return ms;
    }

private:
    std::chrono::steady_clock::time_point t0_;
};

// fn(begin, end) over [0, n) in contiguous pieces on min(hardware threads, 16, KRTRACE_HOST_THREADS) threads (the calling thread takes the first)
template <class F>
inline void parallel_for(int64_t n, F fn)
{
    unsigned hw = std::thread::hardware_concurrency();
    int64_t t = hw == 0 ? 4 : (hw < 16 ? hw : 16);
    if (const char* e = getenv("KRTRACE_HOST_THREADS")) {
        const int v = atoi(e);
        if (v >= 1 && v < t) t = v;
    }
    if (n < (int64_t) 1 << 16) t = 1;
    if (t <= 1) { fn((int64_t) 0, n); return; }
    std::vector<std::thread> others;
    others.reserve((size_t) t - 1);
    for (int64_t i = 1; i < t; ++i) others.emplace_back(fn, n * i / t, n * (i + 1) / t);
    fn((int64_t) 0, n / t);
    for (std::thread& th : others) th.join();
}

}   // namespace krapp

#endif /* KR_APP_COMMON_H_ */
