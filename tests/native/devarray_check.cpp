// Host check of csrc/dev_array.hpp against tests/native/fakehip (hipMalloc / hipFree / hipMemcpy over the heap): ownership,
// moves, uploads, and the build-a-local-then-move pattern of the library's upload functions under a failing allocation.
// Built with -fsanitize=address,undefined where the runtime exists: a leak or a double free fails the run by itself.
//   make -C bsmr-sddmm_amd devarray-check
#include "dev_array.hpp"

#include <cstdio>
#include <cstring>
#include <utility>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

namespace {

struct Record {
    uint32_t a, b, c;
};

// a format the way the library declares them: arrays of different element types and plain fields, no destructor
struct Format {
    uint32_t H = 0;
    DevArray<uint32_t> rows;
    DevArray<uint16_t> lens;
    DevArray<uint8_t> tiles;
    DevArray<Record> items;
};

struct HostFormat {
    uint32_t H = 4;
    std::vector<uint32_t> rows = {1, 2, 3, 4, 5};
    std::vector<uint16_t> lens = {7, 8, 9};
    std::vector<uint8_t> tiles = std::vector<uint8_t>(256, 0xAB);
    std::vector<Record> items = {{1, 2, 3}, {4, 5, 6}};
};

// written like uploadDense: everything goes into a local; the destination and the counter change on success alone
bool uploadFormat(Format& dst, const HostFormat& host, uint64_t& indexBytes) {
    Format f;
    uint64_t bytes = 0;
    f.H = host.H;
    bool ok = devUpload(f.rows, host.rows, bytes) == hipSuccess;
    if (ok) ok = devUpload(f.lens, host.lens, bytes) == hipSuccess;
    if (ok) ok = devUpload(f.tiles, host.tiles, bytes) == hipSuccess;
    if (ok) ok = devUpload(f.items, host.items, bytes) == hipSuccess;
    if (!ok) return false;
    dst = std::move(f);
    indexBytes += bytes;
    return true;
}

template <typename T>
int checkUpload(size_t n) {
    std::vector<T> src(n);
    for (size_t i = 0; i < n; ++i) src[i] = (T)(i * 2654435761u + 17u);
    const long before = fakehip::live;
    {
        DevArray<T> a;
        uint64_t bytes = 5;
        CHECK(devUpload(a, src, bytes) == hipSuccess);
        CHECK(bytes == 5 + n * sizeof(T));
        CHECK(a.count() == n && a.bytes() == n * sizeof(T) && a.get() != nullptr);
        CHECK(std::memcmp(a.get(), src.data(), a.bytes()) == 0);
        CHECK(fakehip::live == before + 1);
    }
    CHECK(fakehip::live == before);
    return 0;
}

int run() {
    // default state, alloc(0), upload of nothing: null, and the allocator is never called
    {
        DevArray<uint32_t> a;
        CHECK(a.get() == nullptr && a.count() == 0 && a.bytes() == 0 && !a);
        CHECK(a.alloc(0));
        CHECK(a.get() == nullptr && a.count() == 0);
        uint64_t bytes = 0;
        CHECK(devUpload(a, std::vector<uint32_t>(), bytes) == hipSuccess);
        CHECK(a.get() == nullptr && bytes == 0);
        CHECK(fakehip::mallocs == 0 && fakehip::live == 0);
    }
    // alloc, move construction, move assignment onto a live array, reset
    {
        DevArray<uint64_t> a;
        CHECK(a.alloc(10));
        CHECK(a.count() == 10 && a.bytes() == 80 && fakehip::live == 1);
        uint64_t* const pa = a.get();
        const uint64_t* viaConversion = a;   // what a kernel launch or hipMemcpy sees
        CHECK(viaConversion == pa);
        DevArray<uint64_t> b(std::move(a));
        CHECK(a.get() == nullptr && a.count() == 0 && b.get() == pa && b.count() == 10 && fakehip::live == 1);
        DevArray<uint64_t> c;
        CHECK(c.alloc(3) && fakehip::live == 2);
        c = std::move(b);   // frees c's three elements
        CHECK(fakehip::live == 1 && c.get() == pa && c.count() == 10 && b.get() == nullptr);
        CHECK(c.alloc(4) && fakehip::live == 1 && c.count() == 4);   // alloc frees what was held
        c.reset();
        CHECK(fakehip::live == 0 && c.get() == nullptr && c.count() == 0);
        c.reset();
        CHECK(fakehip::live == 0);
        // a failed alloc leaves null and reports the error
        CHECK(c.alloc(2) && fakehip::live == 1);
        fakehip::failAfter = 1;
        hipError_t e = hipSuccess;
        CHECK(!c.alloc(5, &e) && e == hipErrorOutOfMemory && c.get() == nullptr && c.count() == 0 && fakehip::live == 0);
    }
    // self-move-assignment is harmless
    {
        DevArray<uint32_t> a;
        CHECK(a.alloc(6));
        uint32_t* const pa = a.get();
        DevArray<uint32_t>& alias = a;
        a = std::move(alias);
        CHECK(a.get() == pa && a.count() == 6 && fakehip::live == 1);
    }
    CHECK(fakehip::live == 0);
    // release / adopt: an array handed on under another element type is still freed once
    {
        DevArray<uint32_t> words;
        CHECK(words.alloc(12 * 5));
        DevArray<Record> records;
        const size_t n = words.bytes() / sizeof(Record);
        records.adopt(reinterpret_cast<Record*>(words.release()), n);
        CHECK(words.get() == nullptr && words.count() == 0 && records.count() == 20 && records.bytes() == 240 && fakehip::live == 1);
    }
    CHECK(fakehip::live == 0);
    // uploads: the same bytes come back, the counter advances by exactly n * sizeof(T)
    for (size_t n : {(size_t)1, (size_t)3, (size_t)1000}) {
        if (checkUpload<uint8_t>(n) || checkUpload<uint16_t>(n) || checkUpload<uint32_t>(n) || checkUpload<uint64_t>(n)) return 1;
    }
    // a struct of four arrays, built in a local and moved out on success
    {
        const HostFormat host;
        const uint64_t want = 5 * 4 + 3 * 2 + 256 + 2 * sizeof(Record);
        Format dst;
        uint64_t indexBytes = 100;
        for (int k = 1; k <= 4; ++k) {   // the k-th allocation fails: nothing reaches the destination, nothing stays allocated
            fakehip::failAfter = k;
            CHECK(!uploadFormat(dst, host, indexBytes));
            CHECK(fakehip::failAfter == 0);
            CHECK(dst.H == 0 && !dst.rows && !dst.lens && !dst.tiles && !dst.items);
            CHECK(indexBytes == 100 && fakehip::live == 0);
        }
        CHECK(uploadFormat(dst, host, indexBytes));
        CHECK(dst.H == 4 && dst.rows.count() == 5 && dst.lens.count() == 3 && dst.tiles.count() == 256 && dst.items.count() == 2);
        CHECK(indexBytes == 100 + want && fakehip::live == 4);
        // a failed rebuild over a built format leaves that format as it was
        uint32_t* const rows = dst.rows.get();
        fakehip::failAfter = 3;
        CHECK(!uploadFormat(dst, host, indexBytes));
        CHECK(dst.H == 4 && dst.rows.get() == rows && indexBytes == 100 + want && fakehip::live == 4);
        // a format in a vector: moved in, freed with it
        std::vector<Format> formats;
        formats.push_back(std::move(dst));
        formats.emplace_back();
        CHECK(formats[0].rows.get() == rows && !dst.rows && fakehip::live == 4);
        formats[0] = Format{};   // (how the library drops a format)
        CHECK(fakehip::live == 0);
    }
    CHECK(fakehip::live == 0);
    return 0;
}

}  // namespace

int main() {
    if (run()) return 1;
    if (fakehip::live != 0) {
        std::fprintf(stderr, "%ld allocations still live\n", fakehip::live);
        return 1;
    }
    std::puts("devarray_check: ok");
    return 0;
}
