// The carrier of host_table.h: the one table-writing kernel of the library.
#include "host_table.h"

#include <algorithm>

namespace l2s {

__global__ __launch_bounds__(256) void host_table_kernel(int32_t* __restrict__ dst, const TableChunk c, int n) {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = c.v[i];
}

int table_upload(int32_t* dst, const int32_t* words, int64_t n_words, hipStream_t s) {
    for (int64_t i0 = 0; i0 < n_words; i0 += TABLE_CHUNK) {
        TableChunk c{};
        const int n = (int)std::min<int64_t>(TABLE_CHUNK, n_words - i0);
        memcpy(c.v, words + i0, (size_t)n * sizeof(int32_t));
        hipLaunchKernelGGL(host_table_kernel, dim3(1), dim3(256), 0, s, dst + i0, c, n);
    }
    L2S_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace l2s
