// Host/device portability macros for the arithmetic headers (mont.cuh, tower.cuh, curve.cuh ...).
//
// The product only ever compiles these headers with hipcc for gfx950.  The same headers also
// compile with plain g++ so that tests/host_harness.cpp can run the *identical* field / tower /
// pairing code on the CPU and diff it against the big-integer oracle while debugging -- that
// harness is test infrastructure and is never linked into libkyberhip.so.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KYB_HD __host__ __device__ __forceinline__
#define KYB_HD_NOINLINE __host__ __device__ __noinline__ inline
#else
#define KYB_HD inline
// host build = tests/host_harness.cpp, one translation unit: the out-of-line boundaries mean nothing there, and gcc
// warns about every function that is both `inline` and `noinline`
#define KYB_HD_NOINLINE inline
#endif

// Register budget (waves per SIMD) of the kernels of a translation unit that name no budget of their own.  Out-of-line
// device functions take the LOOSEST budget of the kernels that reach them, so one kernel without a budget lets every
// shared callee -- and with it every kernel of the unit -- grow to 512 registers: a unit that wants two waves per SIMD
// says so for all of its kernels (-DKYB_TU_WAVES=2).
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 1
#endif

// Per-call flags of the pairing-suite entry points (values mirror include/kyber_hip.h; context.hip static_asserts).
namespace kyb {
constexpr uint32_t FLAG_UNCOMPRESSED = 2u;  // BLS12-381 point inputs are ZCash uncompressed (96 / 192 B)
constexpr uint32_t FLAG_UNCOMPRESSED_OUT = 4u;  // BLS12-381 point outputs of mul are uncompressed too
constexpr uint32_t FLAG_TRUSTED0 = 0x100u;  // point argument i (bit 8 + i) was validated before: skip its checks
KYB_HD bool flag_trusted(uint32_t flags, int arg) { return (flags >> (8 + arg)) & 1u; }

// Kinds of the per-(kind, stream) device workspaces (context.h ctx_workspace).  WS_G1TAB / WS_G2TAB: the ladders' per-lane
// table slabs (pairing_abi.cuh mul_dev; a group policy names its own); WS_IBE: bls12381_ibe.hip's intermediates;
// WS_ED_RING: ed25519_ring.hip, the window tables one call shares; WS_ED_PROOF: ed25519_proof.hip's; WS_ED_COSI: ed25519_cosi.hip's roster, subset tables and T_all; WS_ED_VSS: ed25519_vss.hip's decoded commitments and H tables; WS_ED_ANON: ed25519_anonenc.hip, the window tables of the set one call shares; WS_ED_DSS: ed25519_dss.hip's session hashes, session ids and folded commitments; WS_BDN: bdn_launch.cuh's canonical roster, decoded points, subset tables and partial sums; WS_FB + 2 * suite + group: fixed_base.cuh
enum { WS_MSM = 0, WS_ED = 1, WS_PAIR = 2, WS_LVM = 3, WS_SCALAR = 4, WS_VKEY = 5, WS_G2TAB = 6, WS_G1TAB = 7, WS_IBE = 8, WS_ED_RING = 9, WS_ED_PROOF = 10, WS_ED_COSI = 11, WS_ED_VSS = 12, WS_ED_ANON = 13, WS_BDN = 14, WS_ED_DSS = 15, WS_FB = 16 };

struct DstArg {  // hash-to-curve domain separation tag, passed by value to the kernels (RFC 9380: at most 255 bytes)
    uint8_t b[256];
    uint32_t len;
};
}  // namespace kyb
