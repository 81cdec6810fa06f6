// spans.h — the overlap test of the calls that write caller-held outputs next to caller-held inputs (calibrate.cpp,
// demosaic.cpp): no output may overlap anything the call reads in the same memory space. Host only, no HIP: a host-only
// program checks it (tests/sanitize/demosaic_harness.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace stk {

// The byte ranges a call reads: add every one, seal once, then ask for each output whether it overlaps any of them.
class SpanSet {
public:
    void add(const void* p, size_t bytes) { in_.push_back({(uintptr_t)p, (uintptr_t)p + bytes}); }
    void seal() {
        std::sort(in_.begin(), in_.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
        reach_.resize(in_.size());                          // the furthest end among the spans up to this one
        for (size_t k = 0; k < in_.size(); k++) reach_[k] = std::max(in_[k].hi, k ? reach_[k - 1] : 0);
    }
    bool overlaps(const void* p, size_t bytes) const {
        const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
        const size_t k = std::lower_bound(in_.begin(), in_.end(), hi, [](const Span& s, uintptr_t v) { return s.lo < v; }) - in_.begin();
        return k > 0 && reach_[k - 1] > lo;
    }

private:
    struct Span { uintptr_t lo, hi; };
    std::vector<Span> in_;
    std::vector<uintptr_t> reach_;
};

}  // namespace stk
