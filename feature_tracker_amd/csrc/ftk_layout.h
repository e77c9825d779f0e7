// ftk_layout.h — how a block of bytes is carved into arrays: ONE sequence of take() calls gives every offset, every element type, every
// copy length and the total handed to the block's owner, so they cannot disagree.  Two flavours of the one class, by the boundary a
// slot starts on: 256 bytes (ftk_layout, ftk_slot) for the staging blocks of the host-buffer entry points (device scratch, its pinned
// mirror, a context's workspace), 16 bytes (ftk_layout16, ftk_slot16) for the workspaces a caller owns, which the plans lay out
// (two_view_plan.h and its like) and the entries carve with slot.in(workspace).  Host only, no HIP header:
// host/examples/layout_cli.cpp walks both without a device.
#pragma once

#include <stddef.h>
#include <stdint.h>

// One array of a laid-out block: where it starts (a multiple of Align) and how many elements it holds.
template <class T, size_t Align = 256>
struct ftk_slot {
    size_t offset = 0, count = 0;
    size_t size_bytes() const { return sizeof(T) * count; }                                          // the payload: what a memcpy / a copy of this array moves
    size_t padded_bytes() const { return (size_bytes() + Align - 1) / Align * Align; }                // what it occupies
    T *in(void *base) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + offset); }  // the array inside any block laid out this way
};

// Hands out slots in call order, each on the next Align-byte boundary; a slot of count 0 occupies nothing.  No state but the running
// offset and the flag below.
template <size_t Align>
class ftk_layout_of {
    static_assert(Align != 0 && (Align & (Align - 1)) == 0, "a boundary is a power of two");

public:
    template <class T>
    ftk_slot<T, Align> take(size_t count) {
        if (!ok_ || count > (SIZE_MAX - (Align - 1) - end_) / sizeof(T)) {  // the padded end would wrap: the layout is void from here on
            ok_ = false;
            return {};
        }
        const ftk_slot<T, Align> s{end_, count};
        end_ += s.padded_bytes();
        return s;
    }
    bool ok() const { return ok_; }                       // false: a size wrapped — the caller answers FTK_E_INVALID_ARGUMENT and uses no slot
    size_t bytes() const { return ok_ ? end_ : SIZE_MAX; }  // the padded end of the last slot: what the block must hold (never a small number after a wrap)
    // From the start of `first` to the padded end of `last`: one copy over neighbouring slots.
    template <class A, class B>
    static size_t span_bytes(const ftk_slot<A, Align> &first, const ftk_slot<B, Align> &last) { return last.offset + last.padded_bytes() - first.offset; }

private:
    size_t end_ = 0;
    bool ok_ = true;
};

using ftk_layout = ftk_layout_of<256>;   // staging blocks
using ftk_layout16 = ftk_layout_of<16>;  // caller-owned workspaces
template <class T>
using ftk_slot16 = ftk_slot<T, 16>;
