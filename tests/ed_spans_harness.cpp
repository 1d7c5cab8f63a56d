// kyber_amd/csrc/ed_spans.h compiled for the CPU (test infrastructure, never linked into libkyberhip.so): a stand-alone
// program that tests/test_ed_spans_host.py builds twice, plainly and with -fsanitize=address,undefined, and runs once per
// case.  Usage:  ed_spans_harness <buf|null> off[0] off[1] ... off[n]
// `buf`: the batch's bytes are a heap block of exactly off[n] bytes (byte j holds j * 7 + 1) where off[n] is small, so that
// a read through the rebased view that leaves the caller's buffer is an error under the sanitizer; where off[n] is large
// the pointer is a made-up address that is only displaced, never read.  Prints `refused`, or one line
//   lead=<off[0]> total=<bytes> base=<null | base - bytes> at=<at(out) - out> at_null=<1 if at(nullptr) is null>
//   offsets_bytes=<(n + 1) * 8> same=<1 if every element reads the same bytes through both views> rel=<r0,r1,...>
#include "../kyber_amd/csrc/ed_spans.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using kyb::EdHostSpans;

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const bool null_bytes = !strcmp(argv[1], "null");
    const size_t n = (size_t)argc - 3;
    std::vector<uint64_t> off(n + 1);
    for (size_t i = 0; i <= n; i++) off[i] = strtoull(argv[2 + i], nullptr, 10);

    const bool real = !null_bytes && off[n] <= 4096;
    uint8_t* heap = nullptr;  // exactly off[n] bytes: one more is the sanitizer's
    if (real) {
        heap = (uint8_t*)malloc(off[n] ? off[n] : 1);
        for (uint64_t j = 0; j < off[n]; j++) heap[j] = (uint8_t)(j * 7 + 1);
    }
    const uint8_t* bytes = null_bytes ? nullptr : real ? heap : (const uint8_t*)(uintptr_t)0x10000;

    if (EdHostSpans::offsets_bad(n, bytes, off.data())) {
        puts("refused");
        free(heap);
        return 0;
    }
    const EdHostSpans sp(n, bytes, off.data());
    int same = 1;
    if (real)
        for (size_t i = 0; i < n; i++) {
            const uint64_t len = sp.rel[i + 1] - sp.rel[i];
            if (len != off[i + 1] - off[i] || (len && memcmp(sp.base + sp.rel[i], bytes + off[i], len))) same = 0;
            for (uint64_t j = 0; j < len; j++)
                if (sp.base[sp.rel[i] + j] != (uint8_t)((off[i] + j) * 7 + 1)) same = 0;
        }
    uint8_t* out = (uint8_t*)(uintptr_t)0x20000;  // displaced, never written
    printf("lead=%" PRIu64 " total=%zu ", sp.lead, sp.total);
    if (sp.base)
        printf("base=%" PRIu64, (uint64_t)((uintptr_t)sp.base - (uintptr_t)bytes));
    else
        printf("base=null");
    printf(" at=%" PRIu64 " at_null=%d offsets_bytes=%zu same=%d rel=", (uint64_t)((uintptr_t)sp.at(out) - (uintptr_t)out),
           sp.at(nullptr) == nullptr, sp.offsets_bytes(), same);
    for (size_t i = 0; i <= n; i++) printf("%s%" PRIu64, i ? "," : "", sp.offsets()[i]);
    puts("");
    free(heap);
    return 0;
}
