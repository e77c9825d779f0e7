// ftk_layout.h — how the host-buffer entry points carve a staging block (device scratch, its pinned mirror, a workspace) into
// arrays: ONE sequence of take() calls gives every offset, every copy length and the total handed to the block's owner, so the
// three cannot disagree.  Host only, no HIP header: host/examples/layout_cli.cpp walks it without a device.
#pragma once

#include <stddef.h>
#include <stdint.h>

// One array of a laid-out block: where it starts (a multiple of 256) and how many elements it holds.
template <class T>
struct ftk_slot {
    size_t offset = 0, count = 0;
    size_t size_bytes() const { return sizeof(T) * count; }                                          // the payload: what a memcpy / a copy of this array moves
    size_t padded_bytes() const { return (size_bytes() + 255) / 256 * 256; }                          // what it occupies
    T *in(void *base) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + offset); }  // the array inside any block laid out this way
};

// Hands out slots in call order, each on the next 256-byte boundary; a slot of count 0 occupies nothing.  No state but the running
// offset and the flag below.
class ftk_layout {
public:
    template <class T>
    ftk_slot<T> take(size_t count) {
        if (!ok_ || count > (SIZE_MAX - 255 - end_) / sizeof(T)) {  // the padded end would wrap: the layout is void from here on
            ok_ = false;
            return {};
        }
        const ftk_slot<T> s{end_, count};
        end_ += s.padded_bytes();
        return s;
    }
    bool ok() const { return ok_; }                       // false: a size wrapped — the caller answers FTK_E_INVALID_ARGUMENT and uses no slot
    size_t bytes() const { return ok_ ? end_ : SIZE_MAX; }  // the padded end of the last slot: what the block must hold (never a small number after a wrap)
    // From the start of `first` to the padded end of `last`: one copy over neighbouring slots.
    template <class A, class B>
    static size_t span_bytes(const ftk_slot<A> &first, const ftk_slot<B> &last) { return last.offset + last.padded_bytes() - first.offset; }

private:
    size_t end_ = 0;
    bool ok_ = true;
};
