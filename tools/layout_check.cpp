// Stand-alone host check of the block layout helper (svo_amd/csrc/layout.hpp),
// meant for a sanitizer build on the build machine:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -Isvo_amd/csrc tools/layout_check.cpp -o tools/bin/layout_check
//   tools/bin/layout_check
// Every layout below is measured, then placed into a malloc'ed buffer of exactly
// bytes() -- from the buffer and from the buffer + 1 (the buffer then one byte
// longer) -- and the last byte of every member is written, so an overrun is
// ASan's to report. Exit status 0 only if every member is 256-aligned, inside
// the buffer and clear of the others, both passes visit the same extents, and
// the measuring pass returned null pointers alone.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "layout.hpp"
#include "match_projected.hpp"

using svo::Carver;

namespace {

struct Pose16 {
    float q[4];
};
static_assert(sizeof(Pose16) == 16, "the 16-byte member type");

// A Carver that records what each take() did: the member's start (an offset from
// the first 256-byte boundary at or after the base) and its size.
struct Probe {
    Carver c;
    bool place;
    uintptr_t origin = 0;
    struct Member {
        size_t start, size;
        char* p;
    };
    std::vector<Member> m;
    Probe() : place(false) {}
    explicit Probe(char* base) : c(base), place(true), origin(((uintptr_t)base + 255) & ~(uintptr_t)255) {}
    template <class T>
    T* take(size_t count) {
        T* p = c.take<T>(count);
        const size_t size = sizeof(T) * count;
        // measuring: bytes() is the end from an aligned base, plus the 255 of slack
        const size_t start = place ? (size_t)((uintptr_t)p - origin) : c.bytes() - 255 - size;
        m.push_back({start, size, (char*)p});
        return p;
    }
};

using Layout = std::function<void(Probe&)>;

int failures = 0;
void fail(const char* name, const char* what, size_t i) {
    std::printf("FAIL %s: member %zu %s\n", name, i, what);
    failures++;
}

void check(const char* name, const Layout& layout) {
    Probe meas;
    layout(meas);
    const size_t bytes = meas.c.bytes();
    for (size_t i = 0; i < meas.m.size(); i++)
        if (meas.m[i].p) fail(name, "not null in the measuring pass", i);
    for (size_t shift = 0; shift < 2; shift++) {
        char* buf = (char*)std::malloc(bytes + shift);
        if (!buf) std::exit(2);
        Probe pl(buf + shift);
        layout(pl);
        if (pl.m.size() != meas.m.size()) fail(name, "count differs between the passes", pl.m.size());
        for (size_t i = 0; i < pl.m.size() && i < meas.m.size(); i++) {
            const Probe::Member& a = pl.m[i];
            if ((uintptr_t)a.p % 256) fail(name, "not 256-aligned", i);
            if (a.p < buf + shift || a.p + a.size > buf + shift + bytes) fail(name, "outside the buffer", i);
            if (a.start != meas.m[i].start || a.size != meas.m[i].size) fail(name, "extent differs between the passes", i);
            for (size_t j = 0; j < i; j++)
                if (a.size && pl.m[j].size && a.p < pl.m[j].p + pl.m[j].size && pl.m[j].p < a.p + a.size)
                    fail(name, "overlaps an earlier member", i);
            if (a.size) a.p[a.size - 1] = (char)i;  // ASan sees an overrun
        }
        std::free(buf);
    }
    std::printf("%-28s %3zu members %12zu bytes\n", name, meas.m.size(), bytes);
}

}  // namespace

int main() {
    check("zero count first", [](Probe& p) {
        p.take<int>(0);
        p.take<double>(7);
        p.take<uint8_t>(300);
    });
    check("zero count in the middle", [](Probe& p) {
        p.take<float>(65);
        p.take<double>(0);
        p.take<int>(3);
    });
    check("zero count last", [](Probe& p) {
        p.take<uint8_t>(257);
        p.take<Pose16>(2);
        p.take<float>(0);
    });
    check("one byte", [](Probe& p) { p.take<uint8_t>(1); });
    check("nothing", [](Probe&) {});
    for (int opt = 0; opt < 4; opt++)  // optional members absent and present
        check(opt == 0 ? "optional: none" : opt == 3 ? "optional: both" : "optional: one", [opt](Probe& p) {
            p.take<double>(12 * 5);
            double* res = (opt & 1) ? p.take<double>(2 * 37) : nullptr;
            p.take<float>(2 * 37);
            int* counts = (opt & 2) ? p.take<int>(5) : nullptr;
            p.take<uint8_t>(37);
            (void)res;
            (void)counts;
        });
    check("forty mixed members", [](Probe& p) {
        for (size_t i = 0; i < 40; i++) {
            const size_t n = (i * 7919 + 1) % 613;  // 1 .. 612, odd and even, some below an element of slack
            switch (i % 5) {
                case 0: p.take<uint8_t>(n); break;
                case 1: p.take<int>(n); break;
                case 2: p.take<float>(n + 1); break;
                case 3: p.take<double>(n); break;
                default: p.take<Pose16>(n); break;
            }
        }
    });
    // svo_match_projected's scratch (match_projected.hpp): no keypoint rows, one
    // problem on the smallest grid, and the largest grid
    for (int k = 0; k < 3; k++) {
        const int w = k == 2 ? 1241 : 7, h = k == 2 ? 376 : 5;
        const size_t problems = k == 0 ? 0 : k == 1 ? 1 : 33, rows = k == 0 ? 0 : k == 1 ? 1 : 2001;
        check(k == 0 ? "proj scratch: empty" : k == 1 ? "proj scratch: one" : "proj scratch: 33 x 2001", [=](Probe& p) {
            svo::ProjScratch s;
            svo::proj_scratch_layout(p, s, problems, rows, svo::proj_grid(w, h));
        });
    }
    {  // measured only: 3 << 30 doubles (24 GiB) between two small members must not wrap
        Probe meas;
        meas.take<int>(5);
        meas.take<double>((size_t)3 << 30);
        meas.take<uint8_t>(9);
        const size_t want = 256 + ((size_t)24 << 30) + 9 + 255;
        if (sizeof(size_t) < 8 || meas.c.bytes() != want) fail("large measure", "wrapped", 1);
        std::printf("%-28s %3zu members %12zu bytes\n", "large measure", meas.m.size(), meas.c.bytes());
    }
    std::printf(failures ? "layout_check: %d failure(s)\n" : "layout_check: ok\n", failures);
    return failures ? 1 : 0;
}
