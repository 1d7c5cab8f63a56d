// The shared-inversion encoder of kyber_amd/csrc/ed25519_dev.cuh (ed_encode_chunk) compiled for the CPU (test
// infrastructure, never linked into libkyberhip.so): tests/test_ed_encode_host.py runs every lane of every block of a
// launch, with the prefixes in a lane's own array or in a block's [j][limb][lane] array as the kernels keep them,
// against one field inversion per point.
#include "../kyber_amd/csrc/ed25519_dev.cuh"

#include <string.h>

#include <vector>

using namespace kyb;

extern "C" {

int ede_chunk() { return ENC_CHUNK; }

// out[i] = the 32 bytes of parked point i, one inversion each
void ede_reference(size_t points, const int32_t* proj, uint8_t* out) {
    for (size_t i = 0; i < points; i++) {
        fe X, Y, Z, zi;
        load_fe(X, proj + i * 30);
        load_fe(Y, proj + i * 30 + 10);
        load_fe(Z, proj + i * 30 + 20);
        fe_invert(zi, Z);
        uint32_t w[8];
        ge_encode_with_zinv(w, X, Y, zi);
        memcpy(out + 32 * i, w, 32);
    }
}

// The launch of `records` records of `group` points (1 or 2) in blocks of `block` lanes; lds != 0 keeps the prefixes in
// one array per block (block must be 64 then).  emitted[i] counts the emits of point i, order[i] is its place in its
// lane's sequence.  Returns the number of blocks, or -1 for arguments the harness does not build.
long ede_launch(size_t records, int group, int block, int lds, const int32_t* proj, uint8_t* out, int32_t* emitted,
                int32_t* order) {
    if ((group != 1 && group != 2) || (lds && block != 64)) return -1;
    const size_t span = (size_t)block * ENC_CHUNK;  // points per block: ed_encode_grid
    const size_t blocks = (records * group + span - 1) / span;
    std::vector<int32_t> shared(EncPreLds<64>::WORDS);
    for (size_t b = 0; b < blocks; b++)
        for (int t = 0; t < block; t++) {
            int seq = 0;
            auto emit = [&](size_t i, uint32_t(&w)[8]) {
                memcpy(out + 32 * i, w, 32);
                emitted[i]++;
                order[i] = seq++;
            };
            const size_t first = b * block * (ENC_CHUNK / group) + t;
            EncPreScratch own;
            EncPreLds<64> in_block{shared.data() + t};
            if (group == 1 && lds) ed_encode_chunk<1>(records, proj, first, (size_t)block, in_block, emit);
            if (group == 1 && !lds) ed_encode_chunk<1>(records, proj, first, (size_t)block, own, emit);
            if (group == 2 && lds) ed_encode_chunk<2>(records, proj, first, (size_t)block, in_block, emit);
            if (group == 2 && !lds) ed_encode_chunk<2>(records, proj, first, (size_t)block, own, emit);
        }
    return (long)blocks;
}
}
