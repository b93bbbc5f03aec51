// sl_rows.h -- host side of the kernels that move rows of bytes (sl_rollout.hip, sl_replay.hip): how wide a lane may load
// and store, and the call with the vector type of that width.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

namespace sl {

// the widest of 16 / 8 / 4 / 2 / 1 bytes that divides the row size and every row pointer
inline int row_align(long long bytes, std::initializer_list<const void *> ptrs) {
    unsigned long long bits = (unsigned long long)bytes | 16ull;
    for (const void *p : ptrs) bits |= (unsigned long long)(uintptr_t)p;
    return (int)(bits & (~bits + 1ull));
}

// f(V()) with V the unsigned type of `align` bytes: the row kernels are templates over the element a lane moves
template <typename F>
inline void with_row_type(int align, F &&f) {
    switch (align) {
    case 16: f(uint4()); break;
    case 8: f(uint2()); break;
    case 4: f(uint32_t()); break;
    case 2: f(uint16_t()); break;
    default: f(uint8_t()); break;
    }
}

}  // namespace sl
