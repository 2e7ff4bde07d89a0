// The layout of a block (one allocation cut into typed arrays), stated once: a
// function that takes a Carver and assigns the pointers. It runs twice, on a
// measuring Carver for the block's size and on a placing one, so the two cannot
// disagree. No HIP include: tools/layout_check.cpp builds this header alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace svo {

class Carver {
public:
    Carver() = default;                                                      // measures: take() returns null
    explicit Carver(void* base) : base_((uintptr_t)base), place_(true) {}    // places from any base address
    // the next member: count elements of T at the next 256-byte boundary
    template <class T>
    T* take(size_t count) {
        const uintptr_t a = (base_ + off_ + 255) & ~(uintptr_t)255;
        off_ = (size_t)(a - base_) + sizeof(T) * count;
        return place_ ? (T*)a : nullptr;
    }
    // The block's extent: from any base every member lies inside [base, base + bytes())
    // (the measure counts from an aligned base; another one moves the members up by < 256).
    size_t bytes() const { return place_ ? off_ : off_ + 255; }

private:
    uintptr_t base_ = 0;
    size_t off_ = 0;
    bool place_ = false;
};

// bytes() of the block that `layout` describes
template <class F>
size_t layout_bytes(F&& layout) {
    Carver m;
    layout(m);
    return m.bytes();
}
// the same block placed at `base`
template <class F>
void layout_place(void* base, F&& layout) {
    Carver p(base);
    layout(p);
}

}  // namespace svo
