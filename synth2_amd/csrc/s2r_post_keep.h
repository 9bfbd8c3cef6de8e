// s2r_post_keep.h — what the stages behind the master fader (s2r_post.h) keep on the host from fill to fill: a bounded store of rows
// and the host side of a state that lives on the host or on the device.  Plain vectors and integers, nothing of HIP, so that both are
// checked by a program of their own on the CPU (tests/native/post_keep.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// a fill of `frames` frames behind `pos` frames of the hop under way: the hops it completes, and the frames of the one it leaves under way
inline uint32_t s2r_hop_step(uint32_t pos, uint32_t frames, uint32_t hop, size_t &made) {
    const uint64_t at = (uint64_t)pos + frames;
    made = (size_t)(at / hop);
    return (uint32_t)(at % hop);
}

// The rows a meter keeps, oldest first: at most `max_rows` of `width` floats each; a row past them drops the oldest.
struct S2rRowStore {
    size_t width = 0;                            // (0: no rows, whatever the floats)
    uint32_t max_rows = 0;
    std::vector<float> floats;                   // the rows kept, from row `first` on
    size_t first = 0;
    size_t n_rows() const { return width ? floats.size() / width - first : 0; }
    const float *stored() const { return floats.data() + first * width; }
    void clear() { floats.clear(); first = 0; }
    void shape(size_t row_floats, uint32_t most) { width = row_floats; max_rows = most; clear(); }
    void assign(const float *rows, size_t n) { floats.assign(rows, rows + n * width); first = 0; }       // a checkpoint's: n <= max_rows
    void append(const float *rows, size_t n) {
        floats.insert(floats.end(), rows, rows + n * width);
        if (n_rows() > max_rows) first += n_rows() - max_rows;
        if (first > max_rows) { floats.erase(floats.begin(), floats.begin() + first * width); first = 0; }       // (amortised: once per max_rows rows dropped)
    }
    // the commit of a fill whose kernel left its hops' rows in `rows`: they join the rows kept, and `pos` moves on
    void take(const float *rows, uint32_t &pos, uint32_t frames, uint32_t hop) {
        size_t made;
        pos = s2r_hop_step(pos, frames, hop, made);
        append(rows, made);
    }
};

// The host side of a state that is double-buffered on the device (S2rMirror, s2r_post.h).  The state lives in `host` while host_valid
// — set, reset or restored since the last fill, or fetched — and in the device's copy `cur` otherwise: a fill uploads a valid host
// copy, its kernel writes the other device copy, and the commit flips.  `host` keeps its size, the state's, from set to set: the
// commit leaves its floats stale, not gone.
struct S2rMirrorHost {
    std::vector<float> host;
    bool host_valid = false;
    int cur = 0;
    void set(const float *values, size_t n) { host.assign(values, values + n); host_valid = true; }
    void zero(size_t n) { host.assign(n, 0.0f); host_valid = true; }          // +0.0 everywhere: the meters' state right after a set or a reset
    void off() { host.clear(); host_valid = false; }
    void committed() { cur ^= 1; host_valid = false; }
};
