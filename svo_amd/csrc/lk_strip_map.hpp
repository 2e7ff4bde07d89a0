// lk_multi_kernel's strip map: which of a window's strips (one window column x one
// band of NR rows) a lane of a feature's group owns in its slot k -- stated once,
// for the level setup, the trip loop and the single-group tail, and checked at
// build time (plain constexpr C++: host and device).
//
// A global load costs the texture addresser the same whatever its width (2 to 16
// bytes per lane) and however few lanes are active (tools/ta_load_probe.hip), and
// the level setup is bound by it: the map is chosen so that one load per row
// serves as many of a lane's strips as the widest load covers.
//
//  * dealt (any shape): strip l + LPF k to lane l, slot k; slots past the last
//    strip are dummies (strip 0, zero weights). One load per strip and row.
//  * triples (21 x 21 on 16 lanes, four slots): slots 0, 1, 2 of a lane are the
//    columns c, c + 1, c + 2 of one band -- per row one dword (pixels c .. c + 3,
//    at any byte address) and one 16-byte load (derivative records c .. c + 3)
//    hold all three strips' pairs -- and slot 3 is a single strip, loaded as under
//    the dealt map. 63 = 16 x 3 + 15: sixteen triples, fifteen singles, and the
//    last lane's slot 3 the dummy. Bands 0 and 1: triples at columns 0, 3, .. 12
//    (lanes 0 .. 4, 5 .. 9), singles 15 .. 20 (lanes 0 .. 5, 6 .. 11); band 2:
//    singles 0 .. 2 (lanes 12 .. 14), triples at 3, 6, .. 18 (lanes 10 .. 15).
//    Every lane issues the same loads (no masked group) and reads exactly the
//    pixels and records its strips need: nothing the dealt map does not read.
//    LDS: the trip loop reads entry band NR JRW + col (+ r JRW) of the group's
//    staged region per slot; with JRW = 26 this tiling puts the 16 lanes of every
//    slot on 16 different banks of 32, as the dealt map does.
#pragma once

namespace svo {

struct Strip {
    int col, band;
    bool real;
};

template <int WW, int NB, int LPF>
struct StripMap {
    static constexpr int NSTRIP = WW * NB;
    static constexpr int K = (NSTRIP + LPF - 1) / LPF;  // slots per lane
    static constexpr bool TRIPLES = WW == 21 && NB == 3 && LPF == 16;

    static constexpr Strip at(int l, int k) {
        if constexpr (TRIPLES) {
            if (k < 3) {
                const int band = (l >= 5 ? 1 : 0) + (l >= 10 ? 1 : 0);
                return {3 * (l - 5 * band) + (band == 2 ? 3 : 0) + k, band, true};
            }
            const int band = (l >= 6 ? 1 : 0) + (l >= 12 ? 1 : 0);
            return {l == 15 ? 0 : band == 2 ? l - 12 : 15 + l - 6 * band, l == 15 ? 0 : band, l != 15};
        } else {
            const int sidx = l + LPF * k;
            const bool real = sidx < NSTRIP;
            const int sc = real ? sidx : 0;
            return {sc % WW, sc / WW, real};
        }
    }

    // every real strip exactly once, the other slots dummies, and (triples) a
    // lane's slots 0, 1, 2 real and adjacent columns of one band
    static constexpr bool valid() {
        int seen[NSTRIP] = {};
        int dummies = 0;
        for (int l = 0; l < LPF; l++)
            for (int k = 0; k < K; k++) {
                const Strip s = at(l, k);
                if (s.col < 0 || s.col >= WW || s.band < 0 || s.band >= NB) return false;
                if (s.real)
                    seen[s.band * WW + s.col]++;
                else
                    dummies++;
                if (TRIPLES && k < 3) {
                    const Strip a = at(l, 0);
                    if (!s.real || s.col != a.col + k || s.band != a.band) return false;
                }
            }
        for (int i = 0; i < NSTRIP; i++)
            if (seen[i] != 1) return false;
        return dummies == LPF * K - NSTRIP;
    }
    // the lanes of every slot on different LDS banks (entry rows JRW dwords apart)
    static constexpr bool bank_free(int JRW, int NR) {
        for (int k = 0; k < K; k++) {
            bool used[32] = {};
            for (int l = 0; l < LPF; l++) {
                const Strip s = at(l, k);
                const int b = (s.band * NR * JRW + s.col) % 32;
                if (used[b]) return false;
                used[b] = true;
            }
        }
        return true;
    }
};

static_assert(StripMap<21, 3, 16>::TRIPLES && StripMap<21, 3, 16>::K == 4 && StripMap<21, 3, 16>::valid(),
              "21 x 21: 16 triples, 15 singles, 1 dummy");
static_assert(StripMap<21, 3, 16>::bank_free(26, 7), "21 x 21, 1-px margin: a slot's lanes on 16 banks");
static_assert(!StripMap<11, 1, 16>::TRIPLES && StripMap<11, 1, 16>::valid(), "11 x 11: one strip per lane");

}  // namespace svo
