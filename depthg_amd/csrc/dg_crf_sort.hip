// The two device-wide primitives of the dense-CRF lattice build (dg_crf.hip): a stable LSD radix sort of the packed vertex keys with
// their entry numbers, and an inclusive integer scan of the new-key flags - rocPRIM's header-only implementations, in a unit of their
// own.  Both results are unique (a stable sort, an integer sum), so they do not depend on how the work is scheduled.
#include "dg_device.h"
#include "dg_eval_args.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

size_t dg_crf_sort_temp_bytes(int n) {
    size_t sort_bytes = 0, scan_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (unsigned int)n, 0, 64) != hipSuccess)
        return 0;
    if (rocprim::inclusive_scan(nullptr, scan_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, rocprim::plus<int32_t>())
        != hipSuccess)
        return 0;
    return sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
}

hipError_t dg_crf_sort_pairs(void* temp, size_t temp_bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin, uint32_t* vout,
                             int n, int bits, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, kin, kout, vin, vout, (unsigned int)n, 0, bits, s);
}

hipError_t dg_crf_scan(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out, int n, hipStream_t s) {
    return rocprim::inclusive_scan(temp, temp_bytes, in, out, (size_t)n, rocprim::plus<int32_t>(), s);
}
