// san_room.cpp — s2r_room_reference, s2r_room_state_floats and s2r_room_design of csrc/s2r_rules.cpp under ASan + UBSan
// (tests/test_room_native.py) at the edges of their shapes — no frames, one, two, five, a thousand; the least and the largest delays;
// no output buffer — every buffer allocated at exactly the size s2r.h states, and the answers that need no model.
// Built with -ffp-contract=off.  Prints "room ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "s2r.h"

namespace {

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "san_room.cpp:%d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// a heap block of exactly n floats (n == 0: a pointer that is not null and must not be touched)
struct Buf {
    float *p;
    size_t n;
    explicit Buf(size_t n_, float fill = 0.0f) : p(new float[n_]), n(n_) { for (size_t i = 0; i < n; i++) p[i] = fill; }
    ~Buf() { delete[] p; }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    float &operator[](size_t i) { return p[i]; }
};

uint32_t rng_state = 2468u;
float noise() {                                  // in (-1, 1), never 0
    rng_state = rng_state * 1664525u + 1013904223u;
    return ((float)(rng_state >> 8) + 0.5f) / 8388608.0f - 1.0f;
}
void fill_noise(Buf &b, float scale = 1.0f) { for (size_t i = 0; i < b.n; i++) b[i] = noise() * scale; }
bool same_bits(const float *a, const float *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }

struct Delays { uint32_t cd[S2R_ROOM_COMBS], ad[S2R_ROOM_ALLPASSES], spread; };
const Delays kFlat = {{64, 64, 64, 64, 64, 64, 64, 64}, {64, 64, 64, 64}, 0};
const Delays kSmall = {{64, 65, 71, 79, 83, 89, 97, 101}, {64, 67, 73, 80}, 3};
const Delays kLong = {{8192, 8192, 8192, 8192, 8192, 8192, 8192, 8192}, {8192, 8192, 8192, 8192}, 0};
const Delays kSpread = {{8169, 64, 8169, 64, 8169, 64, 8169, 64}, {64, 8169, 64, 8169}, 23};

int run(const Delays &d, const float *x, uint32_t N, float *state, float *out) {
    return s2r_room_reference(d.cd, d.ad, d.spread, 0.84f, 0.2f, 0.5f, 0.25f, 0.75f, 0.5f, 0.25f, x, N, state, out);
}

// every shape on exact buffers; one call equals two, on bits; a null output moves the state on all the same
void shapes() {
    const uint32_t frames[] = {0u, 1u, 2u, 5u, 1000u};
    for (const Delays *d : {&kFlat, &kSmall, &kLong, &kSpread}) {
        const size_t S = s2r_room_state_floats(d->cd, d->ad, d->spread);
        size_t want = 0;
        for (uint32_t v : d->cd) want += 2u * (size_t)v + d->spread + 2u;
        for (uint32_t v : d->ad) want += 2u * (size_t)v + d->spread;
        CHECK(S == want && S > 0);
        for (uint32_t N : frames) {
            Buf x(2u * (size_t)N), out(2u * (size_t)N), st(S), st2(S), st3(S);
            fill_noise(x); fill_noise(st, 0.25f);
            std::memcpy(st2.p, st.p, S * sizeof(float)); std::memcpy(st3.p, st.p, S * sizeof(float));
            Buf before(S);
            std::memcpy(before.p, st.p, S * sizeof(float));
            CHECK(run(*d, N ? x.p : nullptr, N, st.p, N ? out.p : nullptr) == S2R_OK);
            for (size_t i = 0; i < out.n; i++) CHECK(std::isfinite(out[i]));
            for (size_t i = 0; i < S; i++) CHECK(std::isfinite(st[i]));
            CHECK(run(*d, N ? x.p : nullptr, N, st2.p, nullptr) == S2R_OK);
            CHECK(same_bits(st.p, st2.p, S));
            if (N == 0) { CHECK(same_bits(st.p, before.p, S)); continue; }
            const uint32_t cut = N / 2u;                 // (0 for one frame: an empty first call)
            Buf a(2u * (size_t)cut), b(2u * (size_t)(N - cut)), xa(2u * (size_t)cut), xb(2u * (size_t)(N - cut));
            for (size_t i = 0; i < xa.n; i++) xa[i] = x[i];
            for (size_t i = 0; i < xb.n; i++) xb[i] = x[xa.n + i];
            CHECK(run(*d, cut ? xa.p : nullptr, cut, st3.p, cut ? a.p : nullptr) == S2R_OK);
            CHECK(run(*d, xb.p, N - cut, st3.p, b.p) == S2R_OK);
            CHECK(same_bits(a.p, out.p, a.n) && same_bits(b.p, out.p + a.n, b.n) && same_bits(st3.p, st.p, S));
        }
    }
}

// no model: from silence the first 64 frames are dry * x + 0; with gain 0 and dry 1 the output is the input; in place is the same
void plain_answers() {
    const uint32_t N = 200;
    const size_t S = s2r_room_state_floats(kSmall.cd, kSmall.ad, kSmall.spread);
    Buf x(2u * N), out(2u * N), st(S);
    fill_noise(x);
    CHECK(run(kSmall, x.p, N, st.p, out.p) == S2R_OK);
    for (size_t i = 0; i < 2u * 64u; i++) { const float d = 0.75f * x[i]; CHECK(out[i] == d + 0.0f); }
    Buf st2(S), out2(2u * N);
    CHECK(s2r_room_reference(kSmall.cd, kSmall.ad, kSmall.spread, 0.84f, 0.2f, 0.5f, 0.0f, 1.0f, 0.5f, 0.25f, x.p, N, st2.p, out2.p) == S2R_OK);
    for (size_t i = 0; i < x.n; i++) CHECK(out2[i] == x[i]);
    for (size_t i = 0; i < S; i++) CHECK(st2[i] == 0.0f);
    Buf in_place(2u * N), st3(S);
    for (size_t i = 0; i < x.n; i++) in_place[i] = x[i];
    CHECK(run(kSmall, in_place.p, N, st3.p, in_place.p) == S2R_OK);
    CHECK(same_bits(in_place.p, out.p, out.n) && same_bits(st3.p, st.p, S));
}

// a refusal touches nothing
void refusals() {
    const size_t S = s2r_room_state_floats(kFlat.cd, kFlat.ad, 0);
    Buf x(6), out(6, 9.0f), st(S, 0.25f);
    fill_noise(x);
    Delays bad = kFlat;
    bad.cd[7] = 63;
    CHECK(run(bad, x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE && s2r_room_state_floats(bad.cd, bad.ad, 0) == 0);
    bad = kFlat; bad.ad[3] = 8193;
    CHECK(run(bad, x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE);
    bad = kLong; bad.spread = 1;
    CHECK(run(bad, x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE && s2r_room_state_floats(bad.cd, bad.ad, 1) == 0);
    const float lv[7] = {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f};
    const float wrong[7] = {1.0f, 1.5f, 1.0f, -0.5f, NAN, 2.0f, -1.0f};
    for (int k = 0; k < 7; k++) {
        float l[7];
        std::memcpy(l, lv, sizeof l);
        l[k] = wrong[k];
        CHECK(s2r_room_reference(kFlat.cd, kFlat.ad, 0, l[0], l[1], l[2], l[3], l[4], l[5], l[6], x.p, 3, st.p, out.p) == S2R_ERR_PATCH_RANGE);
    }
    Buf inf(S, 0.25f);
    inf[S - 1] = INFINITY;
    CHECK(run(kFlat, x.p, 3, inf.p, out.p) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_room_reference(nullptr, kFlat.ad, 0, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, x.p, 3, st.p, out.p) == S2R_ERR_INVALID);
    CHECK(s2r_room_reference(kFlat.cd, nullptr, 0, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, x.p, 3, st.p, out.p) == S2R_ERR_INVALID);
    CHECK(run(kFlat, nullptr, 3, st.p, out.p) == S2R_ERR_INVALID);
    CHECK(run(kFlat, x.p, 3, nullptr, out.p) == S2R_ERR_INVALID);
    for (size_t i = 0; i < S; i++) CHECK(st[i] == 0.25f);
    for (size_t i = 0; i < out.n; i++) CHECK(out[i] == 9.0f);
    CHECK(run(kFlat, x.p, 3, st.p, out.p) == S2R_OK);
    uint32_t cd[S2R_ROOM_COMBS], ad[S2R_ROOM_ALLPASSES], spread = 9;
    for (uint32_t &v : cd) v = 9;
    for (uint32_t &v : ad) v = 9;
    CHECK(s2r_room_design(8000.0, 1.0, cd, ad, &spread) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_room_design(44100.0, 6.0, cd, ad, &spread) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_room_design((double)NAN, 1.0, cd, ad, &spread) == S2R_ERR_PATCH_RANGE);
    CHECK(s2r_room_design(48000.0, 1.0, nullptr, ad, &spread) == S2R_ERR_INVALID);
    CHECK(cd[0] == 9 && ad[3] == 9 && spread == 9);
    CHECK(s2r_room_design(44100.0, 1.0, cd, ad, &spread) == S2R_OK);
    CHECK(cd[0] == 1116 && cd[7] == 1617 && ad[0] == 556 && ad[3] == 225 && spread == 23);
    CHECK(s2r_room_design(48000.0, 1.0, cd, ad, &spread) == S2R_OK);
    CHECK(cd[0] == 1215 && ad[3] == 245 && spread == 25 && s2r_room_state_floats(cd, ad, spread) > 0);
}

}  // namespace

int main() {
    shapes();
    plain_answers();
    refusals();
    std::printf("room ok\n");
    return 0;
}
