// What the two four-features-per-wave kernels share (lk_multi_kernel in
// lk_multi.hip, lk_cvq_kernel in lk_cvq.hip): the shape of the groups' staged
// next-image regions and their staging. The kernels' strip map and level setup
// are written out in both: lk_multi_kernel's code is held to the instruction, and
// the compiler schedules it differently as soon as those phases are functions.
#pragma once
#include "lk_device.hpp"

namespace svo {

namespace {

template <int CTRL>
__device__ __forceinline__ int dpp_row_add(int v) {
    // quad_perm / row_ror read a valid lane for every lane: bound_ctrl lets the
    // compiler fold the move into one v_add_u32_dpp (no zero-initialised old value)
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}

// Staging geometry of a JRW x JRH pair region (JRW = 2 mod 4): each lane loads one
// aligned dword of a row (LPR dwords cover the JRW + 1 pixels of a row, RPP rows
// per pass) and writes the four pixel pairs it starts -- entries 4d .. 4d + 3, each
// pixel scaled by 2^kJShift (<= 32640, int16) so that a bilinear J sum carries
// CV_DESCALE(., W_BITS - 5) in its high 16 bits, packed by one permute -- as two
// 8-byte stores (rows are JRW dwords apart: 8- but not 16-byte aligned). The pairs
// take the next lane's dword for their right pixels (ds_bpermute). No store is
// masked and nothing goes to a sink:
//  * a row's last lane (d = LPR - 1) starts only entries JRW - 2, JRW - 1, from its
//    own dword: its second store repeats its first (same address, same data --
//    per-lane permute selectors and address);
//  * lanes past the RPP x LPR slots, and rows past the region in the last pass,
//    repeat a real slot (row RPP - 1, or row JRH - 1): same load, same neighbour
//    (the bpermute source is the real slot's neighbour), same store.
constexpr int kJShift = 7;
static_assert(W_BITS - 5 + kJShift == 16, "J sums must carry their descaled value in bits 16..31");

template <int JRW, int JRH>
struct StageGeom {
    static_assert(JRW % 4 == 2, "rows of 4k + 2 entries: the last lane starts two");
    static constexpr int LPR = (JRW + 2) / 4, RPP = 64 / LPR, NPS = (JRH + RPP - 1) / RPP;
    int lr, d;            // the slot this lane loads and writes (lanes past the slots repeat row RPP - 1)
    int src;              // ds_bpermute byte address of the slot's neighbour
    unsigned selx, sely;  // permute selectors of the second store's pairs (high bytes)
    int hi;               // dword offset of the second store from the first (2, or 0 for the last lane)
    __device__ __forceinline__ explicit StageGeom(int lane) {
        const int l0 = lane / LPR;
        lr = l0 < RPP ? l0 : RPP - 1;
        d = lane - l0 * LPR;
        src = (lr * LPR + d + 1) << 2;
        const bool last = d == LPR - 1;
        selx = last ? 0x010c000cu : 0x030c020cu;  // pixel pairs in the halves' high bytes
        sely = last ? 0x020c010cu : 0x040c030cu;
        hi = last ? 0 : 2;
    }
    __device__ __forceinline__ int row(int q) const {
        const int r = q * RPP + lr;
        return r < JRH ? r : JRH - 1;
    }
    // entries of pass q's row into the region (its row r = row(q))
    __device__ __forceinline__ void write(unsigned* region, int r, unsigned v) const {
        const unsigned nv = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)v);
        unsigned* p = region + r * JRW + 4 * d;
        uint2 a, b;
        // each pixel permuted into the high byte of its half (x 256), then one logical
        // right shift to x 2^kJShift: a fast-rate shift (v_lshrrev; v_lshlrev issues at
        // the slow rate on gfx950, profiles/r05/a_valu_rates.txt)
        constexpr int R = 8 - kJShift;
        a.x = __builtin_amdgcn_perm(nv, v, 0x010c000cu) >> R;
        a.y = __builtin_amdgcn_perm(nv, v, 0x020c010cu) >> R;
        b.x = __builtin_amdgcn_perm(nv, v, selx) >> R;
        b.y = __builtin_amdgcn_perm(nv, v, sely) >> R;
        *reinterpret_cast<uint2*>(p) = a;
        *reinterpret_cast<uint2*>(p + hi) = b;
    }
};

// The staged region (pixel columns xa .. xa + 4 LPR - 1 read as dwords, rows
// y0 .. y0 + JRH - 1) lies inside the padded level.
template <int JRW, int JRH>
__device__ __forceinline__ bool region_in_pad(const ImgLevel& L, int xa, int y0) {
    return xa >= -kPyrPad && y0 >= -kPyrPad && xa + 4 * StageGeom<JRW, JRH>::LPR <= L.w + kPyrPad &&
           y0 + JRH <= L.h + kPyrPad;
}

// one group's region re-staged at (xa, y0) (inside the padding)
template <int W, int H>
__device__ __forceinline__ void stage_padded(unsigned* dst, const ImgLevel& L, int xa, int y0,
                                             const StageGeom<W, H>& g) {
    using G = StageGeom<W, H>;
    const gu8 base = pad_origin(L.data, L.pitch, kPyrPad, 1);
    const unsigned o0 = (unsigned)(xa + kPyrPad + 4 * g.d) + (unsigned)(y0 + kPyrPad) * (unsigned)L.pitch;
    unsigned v[G::NPS];
#pragma unroll
    for (int q = 0; q < G::NPS; q++) v[q] = ldg_off<unsigned>(base, o0 + (unsigned)g.row(q) * (unsigned)L.pitch);
#pragma unroll
    for (int q = 0; q < G::NPS; q++) g.write(dst, g.row(q), v[q]);
}

// FPW features per wave (WW x WH windows, WH a multiple of the strip height NR):
// each group of LPF = 64 / FPW lanes owns one feature; the window's WW x WH / NR
// vertical NR-row strips (21 x 21: 63 strips of 7 rows, 21 columns x 3 row groups;
// 11 x 11: 11 strips of 11 rows) are dealt to the group's lanes, lane l taking
// strips l, l + LPF, ... (slots past the last strip carry zero weights). The per-feature work every
// lane repeats (bilinear weights, bounds / convergence tests, the 2x2 solve) and
// the exact group reduction serve FPW features per instruction. Staged next-
// image regions (margin QJM) for all FPW features share the wave's LDS slice.
// Same exact integer sums and float solve as every other LK kernel.
// Staged region of one group: JRW pair entries x JRH rows. Entry e of row r is the
// pixel pair (x0 + e, x0 + e + 1) with x0 = jx0 & ~3 (the staging reads aligned
// dwords), so an estimate inside the +-QJM margin reads entries up to
// 3 + 2 QJM + WW - 1 and its pair partner: JRW = WW + 2 QJM + 3 entries, not rounded
// up to a multiple of 4 (21 x 21: 26 x 24 entries, 2,496 B; rounding up to 28 cost
// 192 B per group and, with the groups' padding, a wave per CU: 4 x 2,752 B held LK
// at 14 waves per CU, 4 x 2,496 B + the sink admits 16).
// JSTRIDE: the groups' regions lie JSTRIDE bytes apart, the smallest dword count >=
// the region with (dwords mod 32) = 16. ds_read_b32 / ds_read2_b32 bank by (dword
// address) mod 32 over each 32-lane half -- two groups, reading the same strip
// pattern at the same offsets of their own regions: at a multiple of 32 dwords
// apart every read of the pair collided (2-way), 16 banks apart they take disjoint
// halves.
template <int QJM, int WW = 21, int WH = 21, int FPW = 4>
struct MultiShape {
    static_assert(FPW == 4, "four 16-lane groups per wave");
    static constexpr int JRW0 = WW + 2 * QJM + 3;                  // entries the margin needs
    static constexpr int JRW = JRW0 + (6 - JRW0 % 4) % 4;          // rounded up to 4k + 2
    static constexpr int JRH = WH + 1 + 2 * QJM;
    static constexpr int JBYTES = JRW * JRH * 4;
    static constexpr int RES = 16;
    static constexpr int JSTRIDE = (JBYTES / 4 + ((RES - JBYTES / 4) % 32 + 32) % 32) * 4;
    static_assert(JSTRIDE >= JBYTES && (JSTRIDE / 4) % 32 == RES && JSTRIDE - JBYTES < 128, "group stride");
    static_assert(JRW % 4 == 2 && JRW >= JRW0 && JRW < JRW0 + 4, "entries 4k + 2");
};

}  // namespace

}  // namespace svo
