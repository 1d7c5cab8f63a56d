// The IBE hashing of kyber_amd/csrc/bls12381_ibe.cuh compiled for the CPU (test infrastructure, never linked into
// libkyberhip.so): tests/test_ibe_host.py checks H2 / H4 / h3 against hashlib through these entry points.
#include "../kyber_amd/csrc/bls12381_ibe.cuh"

using namespace kyb;

extern "C" {
// out = SHA-256("IBE-H2" || gt), gt 576 bytes
void ibe_h2(const uint8_t* gt, uint8_t* out) {
    uint32_t h[8];
    ibe::h2(h, gt);
    ibe::store_words(out, h, 32);
}
// out = SHA-256("IBE-H4" || sigma[:len])
void ibe_h4(const uint8_t* sigma, int len, uint8_t* out) {
    uint32_t s[8], h[8];
    ibe::load_words(s, sigma, len);
    ibe::h4(h, s, len);
    ibe::store_words(out, h, 32);
}
// r = h3(sigma[:len], msg[:len]) as 32 big-endian bytes; returns 0 or ST_IBE_H3
int ibe_h3(const uint8_t* sigma, const uint8_t* msg, int len, uint8_t* r) {
    uint32_t s[8], m[8], k[8];
    ibe::load_words(s, sigma, len);
    ibe::load_words(m, msg, len);
    const int st = ibe::h3(k, s, m, len);
    ibe::store_words(r, k, 32);
    return st;
}
// out[:len] = a[:len] ^ d[:len], zero beyond
void ibe_xor(const uint8_t* a, const uint8_t* d, int len, uint8_t* out) {
    uint32_t x[8], y[8], z[8];
    ibe::load_words(x, a, 32);
    ibe::load_words(y, d, 32);
    ibe::xor_words(z, x, y, len);
    ibe::store_words(out, z, 32);
}
}
