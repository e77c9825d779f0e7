// layout_cli — walks the layouts of csrc/ftk_layout.h without a device: the 256-byte flavour of the host-buffer entry points' staging
// blocks and the 16-byte flavour of the caller-owned workspaces.
// One command per line on stdin, one line of key=value pairs on stdout for every command except `new` / `new16`:
//   new                      a fresh 256-byte layout
//   new16                    a fresh 16-byte layout
//   take ELEM_BYTES COUNT    the next slot (ELEM_BYTES in 1, 2, 4, 8, 16): offset, payload and padded size of the slot, the layout's flag
//   span I J                 span_bytes from slot I to slot J of this layout (numbered from 0 in take order)
//   total                    bytes() and the flag
// tests/test_layout_cpu.py drives it.
#include <cstdio>
#include <cstring>

#include "ftk_layout.h"

namespace {

struct Bytes16 {
    uint8_t b[16];
};

// One layout of either flavour and every slot taken from it so far, as bytes (same offset, same padded size).
template <size_t Align>
struct Walk {
    ftk_layout_of<Align> L;
    ftk_slot<uint8_t, Align> slots[64];
    size_t n_slots = 0;

    template <class T>
    void take(size_t count) {
        const ftk_slot<T, Align> s = L.template take<T>(count);
        if (n_slots < 64) {
            slots[n_slots++] = {s.offset, s.size_bytes()};
        }
        printf("offset=%zu size=%zu padded=%zu ok=%d\n", s.offset, s.size_bytes(), s.padded_bytes(), L.ok());
    }
    // false: the line is none of this walk's commands
    bool command(const char *line) {
        size_t a = 0, b = 0;
        if (sscanf(line, "take %zu %zu", &a, &b) == 2) {
            switch (a) {
            case 1: take<uint8_t>(b); break;
            case 2: take<uint16_t>(b); break;
            case 4: take<uint32_t>(b); break;
            case 8: take<uint64_t>(b); break;
            case 16: take<Bytes16>(b); break;
            default: return false;
            }
        } else if (sscanf(line, "span %zu %zu", &a, &b) == 2 && a < n_slots && b < n_slots) {
            printf("span=%zu\n", ftk_layout_of<Align>::span_bytes(slots[a], slots[b]));
        } else if (strncmp(line, "total", 5) == 0) {
            printf("total=%zu ok=%d\n", L.bytes(), L.ok());
        } else {
            return false;
        }
        return true;
    }
};

}  // namespace

int main() {
    Walk<256> staging;
    Walk<16> workspace;
    bool sixteen = false;
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        if (strncmp(line, "new", 3) == 0) {
            sixteen = strncmp(line, "new16", 5) == 0;
            staging = {};
            workspace = {};
        } else if (!(sixteen ? workspace.command(line) : staging.command(line))) {
            fprintf(stderr, "layout_cli: cannot parse: %s", line);
            return 2;
        }
    }
    return 0;
}
