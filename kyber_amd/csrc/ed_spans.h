// A host batch of n variable-length elements, as the Ed25519 host entries take one: element i is
// bytes[off[i], off[i + 1]).  Plain C++, nothing from HIP: tests/ed_spans_harness.cpp compiles it for the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace kyb {

struct EdHostSpans {
    // n + 1 offsets, never decreasing; bytes named only where there is a buffer.  For a caller's arguments before
    // anything is built from them.
    static bool offsets_bad(size_t n, const void* bytes, const uint64_t* off) {
        for (size_t i = 0; i < n; i++)
            if (off[i + 1] < off[i]) return true;
        return !bytes && off[n] != off[0];
    }

    // The batch as the device sees it: the bytes from the first element on, and offsets that start at 0
    EdHostSpans(size_t n, const void* bytes, const uint64_t* off)
        : lead(off[0]), total((size_t)(off[n] - off[0])), base(bytes ? (const uint8_t*)bytes + off[0] : nullptr), rel(n + 1) {
        for (size_t i = 0; i <= n; i++) rel[i] = off[i] - lead;
    }

    uint64_t lead;        // off[0]: what the caller's buffer holds in front of the batch
    size_t total;         // bytes of all elements
    const uint8_t* base;  // the first element's byte, nullptr where the caller gave no buffer (every element empty)
    std::vector<uint64_t> rel;  // off[i] - off[0]

    const uint64_t* offsets() const { return rel.data(); }
    size_t offsets_bytes() const { return rel.size() * sizeof(uint64_t); }
    // an output whose elements lie at the input's offsets: where the batch starts in it
    uint8_t* at(uint8_t* out) const { return out ? out + lead : nullptr; }
};

}  // namespace kyb
