// Per-clip tables: the small host-built tables (lengths, prefix sums, per-clip records, the clips each kernel form takes) that an entry point needs in
// device memory before its first real launch.  ONE rule for all of them: the words travel in kernel arguments, TABLE_CHUNK per launch, and are written to
// the call's workspace in stream order - no allocation, no copy from host memory, no synchronisation, no host buffer has to outlive the call, and it works
// under stream capture.  table_upload is that carrier (its one kernel is in host_table.hip); HostTable states a table's layout ONCE: the entry point appends
// typed segments and gets their word offsets back, its workspace sizer appends the same segments without data, so fill, device pointers and size agree.
// Not this mechanism: the tables a consuming kernel takes directly as its own argument and never stores (ClipTab of encoder_kernels.hip, ResizeTab of
// frame_resize.hip, AlignTab of face_align.hip, MelClips of mel_targets.hip), and l2s_pack.hip's uploads from buffers the model owns.
#pragma once
#include "l2s_common.h"

#include <cstring>
#include <type_traits>
#include <vector>

namespace l2s {

constexpr int TABLE_CHUNK = 960;      // words per table-writing launch: one launch carries ~190 vocoder clips, 160 ragged clips, 120 evaluate clips
struct TableChunk { int32_t v[TABLE_CHUNK]; };
static_assert(sizeof(TableChunk) + sizeof(int32_t*) + sizeof(int) <= 4096, "the chunk, the destination and the count fit HIP's 4 KB of kernel arguments");
// dst[0 .. n_words) = words[0 .. n_words) on stream s, ceil(n_words / TABLE_CHUNK) launches; `words` may be freed as soon as the call returns
int table_upload(int32_t* dst, const int32_t* words, int64_t n_words, hipStream_t s);

class HostTable {
public:
    explicit HostTable(bool fill = true) : fill_(fill) {}      // fill = false: sizes only (the workspace sizers) - the same offsets and total, no data
    // Append n elements (src null: zeros, to be written through host<T>()), aligned to the element - 4 bytes, 8 bytes, a record's alignof.  -> word offset
    int64_t i32(const int32_t* src, int64_t n) { return take(src, n, 4, 4); }
    int64_t i64(const int64_t* src, int64_t n) { return take(src, n, 8, 8); }
    template <class T> int64_t rec(const T* src, int64_t n) {
        static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0 && alignof(T) % 4 == 0, "a record of whole 32-bit words");
        return take(src, n, sizeof(T), alignof(T));
    }
    int64_t words() const { return n_; }
    template <class T> T* host(int64_t off) { return fill_ ? reinterpret_cast<T*>(w_.data() + off) : nullptr; }      // valid until the next append
    int upload(int32_t* dst, hipStream_t s) const {
        L2S_REQUIRE(fill_, "host table: a sizes-only table holds nothing to upload");
        return table_upload(dst, w_.data(), n_, s);
    }

private:
    int64_t take(const void* src, int64_t n, int64_t elem, int64_t align) {
        const int64_t a = align / 4, off = (n_ + a - 1) / a * a;
        n_ = off + n * (elem / 4);
        if (fill_) w_.resize((size_t)n_, 0);
        if (fill_ && src && n > 0) memcpy(w_.data() + off, src, (size_t)(n * elem));
        return off;
    }
    std::vector<int32_t> w_;
    int64_t n_ = 0;
    bool fill_;
};
// the device side of a segment: base (the uploaded table, aligned like its widest element) + the offset its append returned
template <class T> inline const T* table_seg(const int32_t* base, int64_t off) { return reinterpret_cast<const T*>(base + off); }

}  // namespace l2s
