// The developer instruments' shared half (a `make EXTRA=-DDG_DEVTOOLS` build; the switches: dg_common.h): the phase stamp a kernel
// takes, and the capture its launcher hands it - a device buffer named by an environment variable, written to that variable's file
// after the launch.  Without DG_DEVTOOLS both are empty, so a launcher uses them without a conditional of its own.
#pragma once
#include <hip/hip_runtime.h>

#ifdef DG_DEVTOOLS
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

// device side: the kernel's argument block `a` carries `stamps`; the threads `pred` selects store the shader clock in `slot`
#define DG_PHASE_STAMP(pred, slot) if (a.stamps && (pred)) a.stamps[slot] = __builtin_amdgcn_s_memtime();

// One capture of one launch: words of T on the device, kept per variable and never freed.  A capture that cannot be set up - the
// variable is not set, the site says it does not fit (`fits`: its grid or its LDS), the buffer cannot be allocated - never fails
// the library call: the launch then runs uninstrumented.
template <class T>
class DgCapture {
    const char* file_ = nullptr;
    T* dev_ = nullptr;

public:
    DgCapture(const char* var, size_t words, bool fits = true) {
        if (!fits || !(file_ = getenv(var))) return;
        static std::mutex mu;
        static std::map<std::string, std::pair<void*, size_t>> bufs;     // variable -> (buffer, bytes): grown when a site asks for more
        std::lock_guard<std::mutex> lock(mu);
        auto& b = bufs[var];
        if (b.second < words * sizeof(T)) {
            void* p = nullptr;
            if (hipMalloc(&p, words * sizeof(T)) != hipSuccess) return;
            b = {p, words * sizeof(T)};
        }
        dev_ = static_cast<T*>(b.first);
    }
    explicit operator bool() const { return dev_ != nullptr; }
    void attach(T*& member) const { if (dev_) member = dev_; }           // (the argument block's pointer stays as it is otherwise)
    void zero(hipStream_t s, size_t words) const { if (dev_) (void)hipMemsetAsync(dev_, 0, words * sizeof(T), s); }
    // after the launch: wait for the stream, bring `words` back, open the file and let `fmt(FILE*, const T*)` write them ...
    template <class F>
    void write(hipStream_t s, size_t words, F fmt, const char* mode = "w") const {
        if (!dev_) return;
        std::vector<T> h(words);
        if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(h.data(), dev_, words * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return;
        if (FILE* fp = fopen(file_, mode)) { fmt(fp, h.data()); fclose(fp); }
    }
    // ... or the words as they are
    void write_raw(hipStream_t s, size_t words) const {
        write(s, words, [words](FILE* fp, const T* h) { fwrite(h, sizeof(T), words, fp); }, "wb");
    }
};

#else

#define DG_PHASE_STAMP(pred, slot)

template <class T>
struct DgCapture {
    DgCapture(const char*, size_t, bool = true) {}
    explicit constexpr operator bool() const { return false; }
    void attach(T*&) const {}
    void zero(hipStream_t, size_t) const {}
    template <class F>
    void write(hipStream_t, size_t, F, const char* = "w") const {}
    void write_raw(hipStream_t, size_t) const {}
};

#endif
