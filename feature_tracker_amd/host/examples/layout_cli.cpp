// layout_cli — walks the staging layout of the host-buffer entry points (csrc/ftk_layout.h) without a device.
// One command per line on stdin, one line of key=value pairs on stdout for every command except `new`:
//   new                      a fresh layout
//   take ELEM_BYTES COUNT    the next slot (ELEM_BYTES in 1, 2, 4, 8, 16): offset, payload and padded size of the slot, the layout's flag
//   span I J                 ftk_layout::span_bytes from slot I to slot J of this layout (numbered from 0 in take order)
//   total                    bytes() and the flag
// tests/test_layout_cpu.py drives it.
#include <cstdio>
#include <cstring>

#include "ftk_layout.h"

namespace {

struct Bytes16 {
    uint8_t b[16];
};

constexpr size_t kMaxSlots = 64;
ftk_slot<uint8_t> slots[kMaxSlots];  // every slot taken so far, as bytes (same offset, same padded size)
size_t n_slots = 0;

template <class T>
void take(ftk_layout &L, size_t count) {
    const ftk_slot<T> s = L.take<T>(count);
    if (n_slots < kMaxSlots) {
        slots[n_slots++] = {s.offset, s.size_bytes()};
    }
    printf("offset=%zu size=%zu padded=%zu ok=%d\n", s.offset, s.size_bytes(), s.padded_bytes(), L.ok());
}

}  // namespace

int main() {
    ftk_layout L;
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        size_t a = 0, b = 0;
        if (strncmp(line, "new", 3) == 0) {
            L = ftk_layout();
            n_slots = 0;
        } else if (sscanf(line, "take %zu %zu", &a, &b) == 2) {
            switch (a) {
            case 1: take<uint8_t>(L, b); break;
            case 2: take<uint16_t>(L, b); break;
            case 4: take<uint32_t>(L, b); break;
            case 8: take<uint64_t>(L, b); break;
            case 16: take<Bytes16>(L, b); break;
            default: fprintf(stderr, "layout_cli: element size %zu\n", a); return 2;
            }
        } else if (sscanf(line, "span %zu %zu", &a, &b) == 2 && a < n_slots && b < n_slots) {
            printf("span=%zu\n", ftk_layout::span_bytes(slots[a], slots[b]));
        } else if (strncmp(line, "total", 5) == 0) {
            printf("total=%zu ok=%d\n", L.bytes(), L.ok());
        } else {
            fprintf(stderr, "layout_cli: cannot parse: %s", line);
            return 2;
        }
    }
    return 0;
}
