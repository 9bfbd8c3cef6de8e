// post_keep.cpp — S2rRowStore, s2r_hop_step and S2rMirrorHost (csrc/s2r_post_keep.h, which includes nothing of HIP) under ASan + UBSan
// (tests/test_rules_native.py).  The row store is held against a model that keeps the last max_rows rows in a std::deque — the count
// and every stored float after each step — over the row widths 1, 18 and S2R_SPECTRUM_ROW(256), max_rows 1, 2 and 5, appends of 0, 1,
// max_rows, max_rows + 1 and 3 max_rows + 1 rows in one call, a run of 4 max_rows + 3 single rows (the compaction fires more than
// once, which is checked), and assign and clear followed by appends.  The position step is held against the quotient and remainder
// in 64 bits, up to pos + frames past 2^32.  The mirror's host side: each transition on its own.  Prints "keep ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "s2r.h"
#include "s2r_post_keep.h"

namespace {

const char *what = "";
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "post_keep.cpp:%d: %s (%s)\n", __LINE__, #cond, what); std::exit(1); } } while (0)

using Row = std::vector<float>;
float next_value = 1.0f;                                 // every float ever handed to a store differs from every other (exact below 2^24)

// a store and its model, fed the same rows
struct Pair {
    S2rRowStore store;
    std::deque<Row> model;
    size_t compactions = 0;
    Pair(size_t width, uint32_t max_rows) { store.shape(width, max_rows); }
    std::vector<float> make(size_t n) {
        std::vector<float> rows(n * store.width);
        for (float &v : rows) { v = next_value; next_value += 1.0f; if (next_value >= 16777216.0f) next_value = 1.0f; }
        return rows;
    }
    void feed_model(const std::vector<float> &rows, size_t n) {
        for (size_t r = 0; r < n; r++) model.emplace_back(rows.begin() + r * store.width, rows.begin() + (r + 1) * store.width);
        while (model.size() > store.max_rows) model.pop_front();
    }
    void same() const {
        CHECK(store.n_rows() == model.size());
        CHECK(store.n_rows() <= store.max_rows);
        CHECK(store.first <= store.max_rows);                    // what the amortised erase bounds: the dropped rows still held
        CHECK(store.floats.size() == (store.first + store.n_rows()) * store.width);
        for (size_t r = 0; r < model.size(); r++) CHECK(std::memcmp(store.stored() + r * store.width, model[r].data(), store.width * sizeof(float)) == 0);
    }
    void append(size_t n) {
        const std::vector<float> rows = make(n);
        const size_t first = store.first;
        store.append(rows.data(), n);                            // (n 0: data() may be null, and nothing is read)
        if (first && !store.first) compactions++;
        feed_model(rows, n);
        same();
    }
    void assign(size_t n) {
        const std::vector<float> rows = make(n);
        store.assign(rows.data(), n);
        model.clear();
        feed_model(rows, n);
        CHECK(store.first == 0);
        same();
    }
    void clear() { store.clear(); model.clear(); CHECK(store.n_rows() == 0 && store.first == 0); same(); }
};

void row_store(size_t width, uint32_t m) {
    what = "appends in one call";
    const size_t counts[5] = {0, 1, m, m + 1u, 3u * m + 1u};
    for (size_t a : counts)
        for (size_t b : counts) {                                // every count on an empty store, and behind every other
            Pair p(width, m);
            CHECK(p.store.n_rows() == 0);
            p.append(a); p.append(b);
        }
    what = "single rows";
    {
        Pair p(width, m);
        for (size_t i = 0; i < 4u * m + 3u; i++) p.append(1);
        CHECK(p.compactions >= 2);
    }
    what = "assign, then appends";
    for (size_t n : {(size_t)0, (size_t)m}) {
        Pair p(width, m);
        p.append(m + 1u);                                        // (the store has dropped a row when the checkpoint's rows come)
        p.assign(n);
        for (size_t a : counts) p.append(a);
        p.assign(n);
        for (size_t i = 0; i < 4u * m + 3u; i++) p.append(1);
    }
    what = "clear, then appends";
    {
        Pair p(width, m);
        p.append(3u * m + 1u); p.clear();
        for (size_t a : counts) p.append(a);
        p.clear();
        for (size_t i = 0; i < 4u * m + 3u; i++) p.append(1);
    }
    what = "a store without a width";
    {
        S2rRowStore off;
        CHECK(off.n_rows() == 0);
        off.shape(0, 0);
        CHECK(off.n_rows() == 0);
    }
}

void hop_step() {
    what = "the position step";
    auto check = [](uint32_t pos, uint32_t frames, uint32_t hop) {
        size_t made = ~(size_t)0;
        const uint32_t left = s2r_hop_step(pos, frames, hop, made);
        const uint64_t at = (uint64_t)pos + (uint64_t)frames;
        CHECK((uint64_t)made == at / hop);
        CHECK((uint64_t)left == at % hop);
        CHECK(left < hop);
    };
    for (uint32_t hop : {1u, 2u, 16u, 32u, 4800u, 1u << 20, 1u << 31, 0xffffffffu})
        for (uint32_t pos : {0u, hop - 1u})
            for (uint64_t frames : {(uint64_t)0, (uint64_t)1, (uint64_t)hop - 1u, (uint64_t)hop, 2u * (uint64_t)hop + 3u, (uint64_t)0xffffffffu}) {
                if (frames > 0xffffffffu) continue;              // (2 hop + 3 of the largest hops is no frame count)
                check(pos, (uint32_t)frames, hop);
            }
    check(1u, 0xffffffffu, 2u);                                  // pos + frames = 2^32 exactly: 2^31 hops and none under way
    check(0xfffffffeu, 0xffffffffu, 0xffffffffu);                // ... and the largest sum there is
    // the store's own step: the rows of the hops a fill completes join the rows kept, and pos moves on
    what = "take";
    Pair p(18, 5);
    uint32_t pos = 31u;
    const uint32_t hop = 32u;
    for (uint32_t frames : {0u, 1u, hop - 1u, hop, 2u * hop + 3u, 7u * hop}) {
        size_t made;
        const uint32_t left = s2r_hop_step(pos, frames, hop, made);
        const std::vector<float> rows = p.make(made);
        p.store.take(rows.data(), pos, frames, hop);
        CHECK(pos == left);
        p.feed_model(rows, made);
        p.same();
    }
}

void mirror_host() {
    const float v[5] = {1.5f, -0.0f, 3.0f, 1e-40f, -7.25f}, w[3] = {9.0f, 8.0f, 7.0f};
    what = "a new mirror";
    {
        S2rMirrorHost m;
        CHECK(!m.host_valid && m.host.empty() && m.cur == 0);
    }
    what = "set";
    {
        S2rMirrorHost m;
        m.set(v, 5);
        CHECK(m.host_valid && m.host.size() == 5 && std::memcmp(m.host.data(), v, sizeof v) == 0 && m.cur == 0);
        m.set(w, 3);                                             // another size: exactly the floats given, none left over
        CHECK(m.host_valid && m.host.size() == 3 && std::memcmp(m.host.data(), w, sizeof w) == 0 && m.cur == 0);
    }
    what = "zero";
    {
        S2rMirrorHost m;
        m.set(v, 5); m.zero(7);
        const float z[7] = {};
        CHECK(m.host_valid && m.host.size() == 7 && std::memcmp(m.host.data(), z, sizeof z) == 0 && m.cur == 0);
    }
    what = "committed";
    {
        S2rMirrorHost m;
        m.set(v, 5); m.committed();
        CHECK(!m.host_valid && m.cur == 1 && m.host.size() == 5);        // (the size stays: the device's copy is that long)
        m.committed();
        CHECK(!m.host_valid && m.cur == 0);
    }
    what = "off";
    {
        S2rMirrorHost m;
        m.set(v, 5); m.off();
        CHECK(!m.host_valid && m.host.empty() && m.cur == 0);
        m.set(v, 5); m.committed(); m.off();
        CHECK(!m.host_valid && m.host.empty() && m.cur == 1);            // (off frees nothing on the device: the copy in turn stays in turn)
    }
    what = "set after committed";
    {
        S2rMirrorHost m;
        m.set(v, 5); m.committed(); m.set(w, 3);
        CHECK(m.host_valid && m.cur == 1 && m.host.size() == 3 && std::memcmp(m.host.data(), w, sizeof w) == 0);
    }
}

}  // namespace

int main() {
    for (size_t width : {(size_t)1, (size_t)18, (size_t)S2R_SPECTRUM_ROW(256)})
        for (uint32_t m : {1u, 2u, 5u}) row_store(width, m);
    hop_step();
    mirror_host();
    std::printf("keep ok\n");
    return 0;
}
