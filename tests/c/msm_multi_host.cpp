// Host side of zl_msm_multi_dev that needs no device (openzl_amd/csrc/zl_msm_multi_plan.h): the argument checks and the chunk planner, swept over the
// shapes the entry point accepts.  A stand-alone program for a sanitizer build (tests/test_msm_multi_host.py compiles it with
// -fsanitize=address,undefined and runs it on the CPU); it walks a host mock of the scratch block through zl_mm_make_layout, the one function
// the driver carves the block with, so an overrun of the planned size is an ASan report and an overflow in the size arithmetic a UBSan one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zl_msm_multi_plan.h"

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

static void check_args() {
    uint64_t out[8];
    const void* sc = out;  // any non-null pointer: the checks never read through it
    CHECK(zl_mm_check_args(100, 0, sc, 100, 100, 3, out) == 0);
    CHECK(zl_mm_check_args(100, 1, sc, 99, 99, 3, out) == 0);
    CHECK(zl_mm_check_args(100, 1, sc, 100, 100, 3, out) == -1);   // first + n past the end
    CHECK(zl_mm_check_args(100, 101, sc, 0, 0, 3, out) == -1);     // first past the end
    CHECK(zl_mm_check_args(100, (size_t)-1, sc, 2, 2, 3, out) == -1);  // first + n wraps
    CHECK(zl_mm_check_args(100, 0, nullptr, 100, 100, 3, out) == -1);
    CHECK(zl_mm_check_args(100, 0, sc, 100, 100, 3, nullptr) == -1);
    CHECK(zl_mm_check_args(100, 0, sc, 100, 99, 3, out) == -1);    // stride below n
    CHECK(zl_mm_check_args(100, 0, sc, 100, (size_t)-1 / 32, 3, out) == -1);  // the last vector's offset wraps
    CHECK(zl_mm_check_args(100, 0, sc, 100, (size_t)-1 / 32, 1, out) == 0);   // ... a single vector has no offset
    CHECK(zl_mm_check_args(100, 0, nullptr, 100, 100, 0, nullptr) == 0);      // count == 0: nothing to do
    CHECK(zl_mm_check_args(100, 100, nullptr, 0, 0, 3, out) == 0);            // n == 0: nothing is read
    CHECK(zl_mm_check_args(100, 0, nullptr, 0, 0, 3, nullptr) == -1);         // ... but the results are written
    CHECK(zl_mm_check_args((size_t)1 << 33, 0, sc, (size_t)1 << 32, (size_t)1 << 32, 1, out) == -1);  // n beyond 32-bit indices
}

static void check_plans() {
    const size_t points[] = {160, 224, 320, 448};  // sizeof(XYZZ) of BN254 G1, BLS12-381 G1, BN254 G2, BLS12-381 G2
    const size_t ns[] = {1, 2, 63, 64, 65, 257, 1000, 2047, 2048, 2049, 4096, 4097, 65536, 100000, (size_t)1 << 24, 0x7fffffffu};
    const size_t counts[] = {1, 2, 3, 64, 65, 130, 1024, 16384, 65535, 65536, 1000000};
    const long overrides[] = {0, 1, 2, 40, 65535, 65536, 1 << 30, -5};
    const size_t budgets[] = {0, 1, 4096, (size_t)1 << 20, ZL_MM_BUDGET};
    for (size_t pb : points)
        for (size_t n : ns)
            for (size_t count : counts)
                for (long ov : overrides)
                    for (size_t budget : budgets) {
                        const size_t fb = pb / 4, ab = pb / 2, ob = pb / 2 - pb / 28;  // F, Affine and canonical-word sizes beside an XYZZ of pb bytes
                        const size_t stage = zl_mm_stage_bytes(pb, ab, fb, ob);
                        const zl_mm_plan p = zl_mm_make_plan(n, count, pb, stage, budget, ov);
                        CHECK(p.slices >= 1 && p.slice_len >= 1 && p.slice_len <= ZL_MM_SLICE);
                        CHECK((n - 1) / p.slice_len < p.slices);                        // every point index lies in one of the slices
                        CHECK((size_t)p.slices * ZL_MM_SLICE < n + ZL_MM_SLICE);         // and no more slices than the slice size asks for
                        CHECK(p.chunk >= 1 && p.chunk <= ZL_MM_MAX_CHUNK && p.chunk <= count);
                        CHECK(p.chunks * p.chunk >= count && (p.chunks - 1) * p.chunk < count);  // the chunks cover every vector, none is empty
                        if (ov > 0 && (size_t)ov <= count && ov <= ZL_MM_MAX_CHUNK) CHECK(p.chunk == (size_t)ov);
                        if (ov <= 0 && p.chunk > 1) CHECK(p.chunk * p.per_vector <= budget);    // the budget bounds the chunk (a single vector may exceed it)
                        CHECK(p.per_vector == (size_t)ZL_MM_WINDOWS * p.slices * pb + stage);
                        CHECK(p.per_vector <= (size_t)-1 / ZL_MM_MAX_CHUNK);            // chunk * per_vector cannot wrap
                        const zl_mm_layout l = zl_mm_make_layout(p, pb, ab, fb, ob);
                        CHECK(l.bad + 4 <= l.part && l.part < l.res && l.res < l.aff && l.aff < l.prefix && l.prefix < l.words && l.words < l.total);
                        CHECK(l.total == 64 + p.chunk * p.per_vector);                  // what the driver asks the scratch slot for
                    }
    const zl_mm_plan none = zl_mm_make_plan(0, 5, 224, 500, ZL_MM_BUDGET, 0), none2 = zl_mm_make_plan(5, 0, 224, 500, ZL_MM_BUDGET, 0);
    CHECK(none.chunks == 0 && none.chunk == 0 && none2.chunks == 0);
}

// the driver's walk over a call: chunk by chunk, every (vector, window, slice) partial and every staging record is written through the shared layout into a
// block of exactly layout.total bytes
static void walk_block() {
    const struct { size_t pb, ab, fb, ob; } groups[] = {{160, 80, 40, 64}, {224, 112, 56, 96}, {320, 160, 80, 128}, {448, 224, 112, 192}};  // BN254 G1, BLS12-381 G1, BN254 G2, BLS12-381 G2
    const struct { size_t n, count; long ov; } cases[] = {{257, 130, 40}, {2100, 3, 0}, {1000, 65, 64}, {65, 5, 2}, {5000, 7, 3}};
    for (const auto& g : groups)
        for (const auto& c : cases) {
            const zl_mm_plan p = zl_mm_make_plan(c.n, c.count, g.pb, zl_mm_stage_bytes(g.pb, g.ab, g.fb, g.ob), ZL_MM_BUDGET, c.ov);
            const zl_mm_layout l = zl_mm_make_layout(p, g.pb, g.ab, g.fb, g.ob);
            std::vector<unsigned char> block(l.total);
            size_t seen = 0;
            for (size_t c0 = 0; c0 < c.count; c0 += p.chunk) {
                const size_t ch = c.count - c0 < p.chunk ? c.count - c0 : p.chunk;
                memset(block.data() + l.bad, 0, 4);
                for (size_t v = 0; v < ch; v++) {
                    for (size_t w = 0; w < ZL_MM_WINDOWS; w++)
                        for (size_t s = 0; s < p.slices; s++) memset(block.data() + l.part + ((v * ZL_MM_WINDOWS + w) * p.slices + s) * g.pb, 0x5a, g.pb);
                    memset(block.data() + l.res + v * g.pb, 1, g.pb);
                    memset(block.data() + l.aff + v * g.ab, 2, g.ab);
                    memset(block.data() + l.prefix + v * g.fb, 3, g.fb);
                    memset(block.data() + l.words + v * g.ob, 4, g.ob);
                    seen++;
                }
            }
            CHECK(seen == c.count);
        }
}

int main() {
    check_args();
    check_plans();
    walk_block();
    printf(failures ? "msm_multi_host: %d FAILED\n" : "msm_multi_host: OK\n", failures);
    return failures ? 1 : 0;
}
