// post_route_eq.cpp — s2r_post_route_eq (csrc/s2r_post_route.h, which includes nothing of HIP) over every call there is, under ASan +
// UBSan (tests/test_eq_native.py): the 24 routes of post_route.cpp — bus fills x the 8 subsets of running stem stages, master fills x
// 8 subsets x limiter on or off, each for both values of `stems` —, each without and with the EQ.  Without it the function changes
// nothing.  With it the EQ reads its own staging buffer and writes where the combine would have written, the combine is redirected
// into the EQ's buffer, and every other pointer is as it was.  Prints "route eq ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "s2r_post_route.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "post_route_eq.cpp:%d: %s (%s)\n", __LINE__, #cond, what); std::exit(1); } } while (0)

// the eight buffers of a call
enum Buf { CH, DL, FX, MS, LI, BO, OH, EQ, N_BUF };      // chorus, delay and fx stages, master_stage, limiter_in, bus_out_dev, out_host_dev, the EQ's stage

bool same_but_head(const S2rPostRoute &a, const S2rPostRoute &b) {       // everything but combine_out and the eq pair
    for (int k = 0; k < S2R_STEM_STAGES; k++) if (a.stem[k].in != b.stem[k].in || a.stem[k].out != b.stem[k].out) return false;
    return a.master_in == b.master_in && a.master_out == b.master_out && a.master_stems == b.master_stems && a.limiter_in == b.limiter_in &&
           a.limiter_out == b.limiter_out;
}

}  // namespace

int main() {
    float cells[N_BUF] = {};                             // one float per buffer, never touched
    float *const stage[S2R_STEM_STAGES] = {cells + CH, cells + DL, cells + FX};
    char what[112] = "a panned call";
    {
        S2rPostCall call;                                // no buses, no route: the EQ flag changes nothing
        call.frames = 64; call.eq = true;
        const S2rPostRoute r = s2r_post_route_eq(call, s2r_post_route(call, stage, cells + MS, cells + LI, cells + BO, cells + OH), cells + EQ);
        CHECK(!r.combine_out && !r.eq.in && !r.eq.out && !r.master_in && !r.limiter_in);
    }
    CHECK(!S2rPostCall{}.eq);                            // off unless prepare finds an EQ
    int routes = 0, calls = 0;
    for (int master = 0; master < 2; master++)
        for (int subset = 0; subset < 1 << S2R_STEM_STAGES; subset++)
            for (int limited = 0; limited <= master; limited++) {
                for (int stems = 0; stems <= master; stems++)
                    for (int eq = 0; eq < 2; eq++) {
                        S2rPostCall call;
                        call.n_buses = 3; call.frames = 64; call.master = master != 0; call.stems = stems != 0; call.limited = limited != 0; call.eq = eq != 0;
                        for (int k = 0; k < S2R_STEM_STAGES; k++) call.on[k] = (subset >> k & 1) != 0;
                        std::snprintf(what, sizeof what, "%s fill, stages %d%d%d, limiter %d, stems %d, eq %d", master ? "master" : "bus", (int)call.on[0],
                                      (int)call.on[1], (int)call.on[2], limited, stems, eq);
                        const S2rPostRoute plain = s2r_post_route(call, stage, cells + MS, cells + LI, cells + BO, cells + OH);
                        CHECK(!plain.eq.in && !plain.eq.out);                    // s2r_post_route itself knows nothing of the EQ
                        const S2rPostRoute r = s2r_post_route_eq(call, plain, cells + EQ);
                        CHECK(same_but_head(r, plain));
                        if (!eq) {
                            CHECK(std::memcmp(&r, &plain, sizeof r) == 0);       // (all pointers, no padding: the whole struct)
                        } else {
                            CHECK(r.eq.in == cells + EQ);
                            CHECK(r.combine_out == r.eq.in);
                            CHECK(r.eq.out == plain.combine_out && r.eq.out != nullptr && r.eq.out != r.eq.in);
                            // the head of the chain: the first running stem stage's buffer, else the master's stage, else the pinned output
                            float *head = call.master ? cells + MS : cells + BO;
                            for (int k = S2R_STEM_STAGES - 1; k >= 0; k--) if (call.on[k]) head = stage[k];
                            CHECK(r.eq.out == head);
                        }
                        calls++;
                    }
                routes++;
            }
    std::snprintf(what, sizeof what, "all calls");
    CHECK(routes == 24 && calls == 2 * (8 + 8 * 2 * 2));
    static_assert(sizeof(S2rPostRoute) == (8 + 2 * S2R_STEM_STAGES) * sizeof(float *), "S2rPostRoute is pointers alone");
    std::printf("route eq ok\n");
    return 0;
}
