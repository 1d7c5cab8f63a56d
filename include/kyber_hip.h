/*
 * kyber_hip.h -- C ABI of libkyberhip.so, the MI355X (gfx950) batched
 * group-arithmetic engine that sits behind dedis/kyber's kyber.Point.Mul /
 * pairing.Suite hot path.
 *
 * This is what a cgo binding in the reference would import (see INTEGRATION.md
 * for the Go stub).  Plain pointers and sizes only.
 *
 * Conventions
 *   - every entry point returns 0 on success, <0 on a call-level error
 *     (KYB_E_*); kyb_last_error() gives a message for the calling thread.
 *   - wire formats are exactly the reference's MarshalBinary encodings;
 *     element-major, densely packed.
 *   - where decoding an input can fail (UnmarshalBinary returning an error in
 *     the reference) the call takes `status[n]`: 0 = ok, KYB_ST_* otherwise,
 *     and the corresponding output element is all-zero bytes.
 *   - "*_dev" variants take DEVICE pointers (already resident in HBM) and a
 *     hipStream_t passed as void* (NULL = default stream); they only enqueue
 *     work and never synchronise.  The host variants copy in, run, copy out
 *     and synchronise.
 *   - all entry points are thread-safe; state is a per-device context that is
 *     created on first use on the calling thread's current HIP device.
 *
 * TIMING: BY DEFAULT NOTHING IN THIS LIBRARY IS CONSTANT-TIME.  Results equal the
 * reference's on every input, but window tables are indexed by scalar digits
 * (through L2), exceptional additions branch, field inversion is a
 * data-dependent loop and KYB_F_VARTIME skips leading zero windows.  The one
 * exception is opt-in: KYB_F_UNIFORM on the Ed25519 multiplications (below).  A suite
 * built on it belongs in suites/all_vartime.go only and must not be offered
 * where suites.RequireConstantTime (suites/suites.go:67) is expected to hold
 * (the reference's default Ed25519 Mul scans its table with CMove,
 * group/edwards25519/ge.go:419-435).  See INTEGRATION.md section 2b.
 */
#ifndef KYBER_HIP_H
#define KYBER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KYB_OK 0
#define KYB_E_ARG (-1)    /* bad argument (NULL pointer, bad flags) */
#define KYB_E_HIP (-2)    /* a HIP runtime call failed */
#define KYB_E_NODEV (-3)  /* no usable gfx950 device */
#define KYB_E_ALLOC (-4)  /* workspace allocation failed */
#define KYB_E_EXHAUSTED (-5) /* kyb_ed25519_xof_pick: the fixed window of candidate draws held fewer than n scalars */

#define KYB_ST_OK 0
#define KYB_ST_BAD_POINT 1 /* encoding is not a curve point (reference: UnmarshalBinary error) */
#define KYB_ST_NOT_IN_SUBGROUP 2
#define KYB_ST_IBE_CHECK 3 /* encrypt/ibe decryption: rP != U ("invalid proof: rP check failed", ibe.go:127-130) */
#define KYB_ST_IBE_H3 4    /* encrypt/ibe: h3's rejection sampling found no scalar in 65 534 tries ("rejection sampling
                              failure", ibe.go:278-280; unreachable in practice, defined all the same) */
#define KYB_ST_SIG_NONCANONICAL 5 /* Ed25519 verify: S >= l, or y >= p in R or in the public key (eddsa.go:158-206) */
#define KYB_ST_SIG_SMALL_ORDER 6  /* Ed25519 verify: R or the public key is one of the eight points of small order */
#define KYB_ST_DLEQ_CHALLENGE 7  /* Ed25519 dleq_verify: the proof's challenge is not the expected one (pvss.go:154-157,
                                    268-270: ErrGlobalChallengeVerification / ErrDecShareChallengeVerification) */
#define KYB_ST_PICK_EXHAUSTED 8  /* Ed25519 dleq: Scalar.Pick found no scalar below l in 128 draws of the XOF (probability
                                    2^-128; unreachable in practice, defined all the same) */
#define KYB_ST_ECIES_SHORT 9     /* encrypt/ecies Decrypt: the ciphertext is shorter than R and a tag, 48 bytes
                                    (ecies.go:85-87; 32..47 bytes fail in Open, ecies.go:111) */
#define KYB_ST_ECIES_AUTH 10     /* encrypt/ecies Decrypt: AES-GCM's tag does not match (ecies.go:111) */
#define KYB_ST_ANON_SHORT 11     /* sign/anon Decrypt: "ciphertext too short" -- fewer than 32 bytes (enc.go:55-57), than the
                                    header of 32 + 32 ring (enc.go:70-72) or than the header and a MAC (enc.go:175-177) */
#define KYB_ST_ANON_INVALID 12   /* sign/anon Decrypt: "invalid ciphertext" -- x B is not X (enc.go:85-88) or the regenerated
                                    header is not the ciphertext's (enc.go:97-99) */
#define KYB_ST_ANON_MAC 13       /* sign/anon Decrypt: "invalid ciphertext: failed MAC check" (enc.go:188-190) */
#define KYB_ST_DSS_INDEX 14      /* sign/dss ProcessPartialSig: "dss: partial signature with invalid index" -- the index is not
                                    below the number of participants (ErrInvalidSignatureIndex, dss.go:142-145) */
#define KYB_ST_DSS_SIG 15        /* sign/dss ProcessPartialSig: the partial signature's Schnorr signature passes its byte-level
                                    checks and fails the equation ("schnorr: invalid signature", dss.go:147-149) */
#define KYB_ST_DSS_SESSION 16    /* sign/dss ProcessPartialSig: "dss: session id do not match" (dss.go:152-154) */
#define KYB_ST_DSS_PARTIAL 17    /* sign/dss ProcessPartialSig: "dss: partial signature not valid" -- V B is not
                                    randomPoly.Eval(I) + h longPoly.Eval(I) (dss.go:160-169) */
#define KYB_ANON_MAX_RING 4096   /* sign/anon Encrypt / Decrypt: the largest anonymity set one call takes -- an element's
                                    ring + 1 lanes fit one piece of the batch, and the tables of a set the batch shares
                                    take 1 280 B a key of workspace */

/* flags */
#define KYB_F_VARTIME 1u /* Ed25519: geScalarMultVartime semantics (all 256 scalar bits honoured,
                            group/edwards25519/ge_mult_vartime.go:11) and leading zero
                            windows skipped per wave. Default = the VALUE semantics of the reference's
                            constant-time path ge.go:443 incl. its >= 2^255 behaviour (not its timing). */

#define KYB_F_UNIFORM 8u /* Ed25519 mul_base / mul / mul_same_base: scalar-INDEPENDENT memory addresses and control flow --
                            the access pattern of the reference's default (constant-time) Mul, group/edwards25519/ge.go:352-371,
                            419-435: every window reads ALL eight table candidates and keeps one by mask, the sign is a
                            conditional move, no window is skipped; same value semantics as the default (incl. >= 2^255).
                            For secret scalars: PriPoly.Commit's coefficients (share/poly.go:143-149), signing nonces
                            (sign/eddsa/eddsa.go), DH.  mul_same_base builds the base's table at any batch size.  Costs
                            ~2x on the fixed-base path (64 additions instead of 32) -- measured, DESIGN.md.  Exclusive with
                            KYB_F_VARTIME.  It removes the digit-indexed loads and the scalar-dependent schedule; the
                            library makes no formal constant-time claim (see TIMING above). */

#define KYB_F_DLEQ_FS 16u /* kyb_ed25519_dleq_verify: C[i] must equal the Fiat-Shamir challenge derived on the device from
                             (xG, xH, VG, VH)[i], the order NewDLEQProof (dleq.go:57-79) and VerifyDecShare
                             (pvss.go:250-270) hash in.  Exclusive with expect_c. */

/* Pairing-suite calls (trailing `flags` argument of mul / msm / pair / pair_check / verify):
 *  KYB_F_UNCOMPRESSED  BLS12-381 point INPUTS are ZCash uncompressed affine (G1 96 B x||y, G2 192 B
 *                      x.c1||x.c0||y.c1||y.c0): no square root (the `_aff` form of SURVEY.md 8b).  Outputs stay
 *                      compressed.  bn256's wire format is already uncompressed: the flag changes nothing there.
 *  KYB_F_TRUSTED(i)    point argument i (0-based, in declaration order) holds points that were validated before --
 *                      outputs of this library or of an earlier UnmarshalBinary, as every kyber.Point handed to
 *                      Mul / Pair already is in the reference (validation happens once, in UnmarshalBinary,
 *                      kilic/g1.go:127-131) -- so the subgroup check (and, for uncompressed input, the curve-equation
 *                      check) is skipped.  Precondition, not a check: a point outside the subgroup then gives a
 *                      result the reference could never produce.  bn256 has no subgroup check to skip. */
#define KYB_F_UNCOMPRESSED 2u
#define KYB_F_UNCOMPRESSED_OUT 4u /* g1/g2 mul and mul_same_base: write uncompressed outputs (96 / 192 B) as well, so a
                                     pipeline can keep points in the form that needs no square root; bn256: no-op */
#define KYB_F_SCALAR_BITS(b) ((uint32_t)(b) << 16) /* *_msm only: every scalar is below 2^b (1 <= b <= 256) -- the
                                     128-bit coefficients of sign/bdn (bdn.go:29-63) run half the windows.  Bits at
                                     and above b are IGNORED (the result is sum (k_i mod 2^b) P_i).  BLS12-381 G1,
                                     which splits full-length scalars into 127-bit halves, honours it for b <= 160
                                     (plain windows) and takes no notice above. */
#define KYB_F_SCALAR_BITS_MASK (0x1ffu << 16)
#define KYB_F_TRUSTED(i) (0x100u << (i))
#define KYB_F_TRUSTED_ALL 0xF00u /* the four point arguments of pair_check; calls with fewer point arguments reject the extra bits */

int kyb_version(void);
const char *kyb_last_error(void);

/* Number of visible devices; creates nothing. */
int kyb_device_count(void);
/* Eagerly create the context (tables, workspace) for the current HIP device. */
int kyb_init(void);
/* Release every per-device context. */
int kyb_shutdown(void);

/* ---- several GPUs of one node behind the same calls (the reference's callers are single-process
 * loops -- share/poly.go:143-149, sign/bdn/bdn.go:126-161 -- so they need ONE call, not one process per GPU).
 * After kyb_init_devices(ndev) (devices 0 .. ndev-1) or kyb_set_devices(list) every HOST-BUFFER batch entry point of
 * at least kyb_set_shard_threshold() units (default 16384) is cut into `ndev` contiguous slices by the rule of
 * kyb_shard_range (sizes differ by at most one), one host thread + device context per slice, no traffic between
 * devices; kyb_*_msm shards the points, runs the whole Pippenger pipeline per device and adds the ndev encoded partial
 * points at the end (<= 129 bytes per device cross the host, bucket arrays never move).  A device may be listed more
 * than once (its slices then run one after the other; used by the tests on a one-GPU box).  ndev = 0 / an empty list
 * restores single-device behaviour.  The `_dev` entry points are unaffected.  Results do not depend on the device
 * set. */
int kyb_init_devices(int ndev);
int kyb_set_devices(const int *devices, int ndev);
int kyb_get_devices(int *out, int cap); /* returns the number of shards configured (0: single device) */
int kyb_set_shard_threshold(size_t min_units);
void kyb_shard_range(size_t n, int rank, int world, size_t *lo, size_t *hi);
/* The `_dev` entry points keep one grow-only device workspace per (kind of call, stream) so that calls on different
 * streams never share scratch.  A caller that destroys a stream calls this first (current device): waits for the
 * stream and frees the workspaces tied to that handle.  Never needed for long-lived streams or the host-buffer calls. */
int kyb_stream_release(void *stream);

/* ------------------------------------------------------------------ Ed25519
 * scalars: 32-byte little-endian, taken as plain 256-bit integers (never
 * reduced mod l: group/edwards25519/scalar.go:226-233).
 * points : 32-byte compressed (group/edwards25519/ge.go:99-150).           */

/* out[i] = scalars[i] * B.   Replaces (*point).Mul(s, nil) ->
 * geScalarMultBase (group/edwards25519/point.go:243, ge.go:373) + MarshalBinary. */
int kyb_ed25519_mul_base(size_t n, const uint8_t *scalars, uint8_t *out, uint32_t flags);
int kyb_ed25519_mul_base_dev(size_t n, const void *d_scalars, void *d_out, uint32_t flags, void *stream);

/* out[i] = scalars[i] * points[i].   Replaces UnmarshalBinary + (*point).Mul(s, A)
 * -> geScalarMult / geScalarMultVartime (point.go:235-258, ge.go:443,
 * ge_mult_vartime.go:11) + MarshalBinary. */
int kyb_ed25519_mul(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t *out,
                    uint8_t *status, uint32_t flags);
int kyb_ed25519_mul_dev(size_t n, const void *d_scalars, const void *d_points, void *d_out,
                        void *d_status, uint32_t flags, void *stream);

/* out[i] = scalars[i] * point  (one shared base).  Replaces the loop of
 * share.PriPoly.Commit (share/poly.go:143-149).  If the point does not decode
 * every status[i] is KYB_ST_BAD_POINT and every output is zero. */
int kyb_ed25519_mul_same_base(size_t n, const uint8_t *scalars, const uint8_t point[32],
                              uint8_t *out, uint8_t *status, uint32_t flags);

/* out[i] = a[i] + b[i]: (*point).Add (group/edwards25519/point.go:216-223 -> ge.go:183), both operands
 * unmarshalled with the reference's rules: bit 255 is the sign of x, y >= p is reduced, "-0" (x = 0 with the sign set)
 * is accepted, the eight points of small order are points like any other; out[i] is the canonical encoding of the sum.
 * status[i] is KYB_ST_BAD_POINT and out[i] zero bytes where either operand has no x.  status (d_status) may be NULL:
 * the outputs are the same, zero bytes on the rejected elements included.  Nothing is written past element n - 1;
 * n = 0 is KYB_OK and touches nothing; a NULL a, b or out with n > 0 is KYB_E_ARG. */
int kyb_ed25519_add(size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *status);
int kyb_ed25519_add_dev(size_t n, const void *d_a, const void *d_b, void *d_out, void *d_status, void *stream);

/* ok[i] = 1 iff VerifyWithChecks(pubkeys[i], msgs[i], sigs[i]) == nil: sign/eddsa VerifyWithChecks (eddsa.go:143-229)
 * and, on this curve, sign/schnorr VerifyWithChecks (schnorr.go:84-160: the same checks in another order, the same
 * bytes R || A || msg hashed, the same equation S B = R + h A) for a batch, one lane program per signature: the
 * byte-level checks, h = SHA-512(R || A || msg) mod l, one variable-base ladder on -A with the fixed-base comb added
 * into the same accumulator, and encode(S B - h A) compared with R's bytes.
 * pubkeys: n x 32 bytes; sigs: n x 64 bytes (R || S); message i is msgs[msg_off[i] .. msg_off[i + 1]), n + 1 offsets.
 * status may be NULL.  status[i], the reference's order of checks as precedence: KYB_ST_SIG_NONCANONICAL (S, R or A
 * not canonical), KYB_ST_SIG_SMALL_ORDER (R or A), KYB_ST_BAD_POINT (A does not decode), otherwise 0: the verdict
 * came from the equation.  An R that is canonical but not a curve point is never decompressed: it lands there too,
 * with status 0 and ok = 0 (it can equal no point's encoding), also when A would fail a later check.
 * flags must be 0.  Host variant: offsets that decrease (the only way one can run past msg_off[n], the end of the
 * buffer) are KYB_E_ARG.  _dev: device pointers, pubkeys and sigs 16-byte aligned, offsets are the caller's contract
 * (a decreasing pair is read as an empty message). */
int kyb_ed25519_verify(size_t n, const uint8_t *pubkeys, const uint8_t *msgs, const uint64_t *msg_off,
                       const uint8_t *sigs, uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_ed25519_verify_dev(size_t n, const void *d_pubkeys, const void *d_msgs, const void *d_msg_off,
                           const void *d_sigs, void *d_ok, void *d_status, uint32_t flags, void *stream);

/* out[i] = a[i] * P[i] + b[i] * Q[i] by Straus-Shamir (two window tables, one chain of doublings, one encoding): the
 * shape of every sigma-protocol check, proof/dleq Proof.Verify (dleq.go:160-172: vG == r G + c xG, vH == r H + c xH).
 * Byte-identical to kyb_ed25519_add(kyb_ed25519_mul(a, P), kyb_ed25519_mul(b, Q)) under the same flag for every
 * 32-byte scalar (unreduced scalars and the >= 2^255 behaviour of kyb_ed25519_mul included).  flags: 0 or
 * KYB_F_VARTIME; KYB_F_UNIFORM is KYB_E_ARG.  status[i] (may be NULL) is KYB_ST_BAD_POINT and out[i] zero if either
 * point does not decode. */
int kyb_ed25519_mul2(size_t n, const uint8_t *a, const uint8_t *P, const uint8_t *b, const uint8_t *Q, uint8_t *out,
                     uint8_t *status, uint32_t flags);
int kyb_ed25519_mul2_dev(size_t n, const void *d_a, const void *d_P, const void *d_b, const void *d_Q, void *d_out,
                         void *d_status, uint32_t flags, void *stream);

/* c[i] = Scalar.Pick(suite.XOF(SHA-256(xG[i] || xH[i] || vG[i] || vH[i]))): the Fiat-Shamir challenge of proof/dleq
 * NewDLEQProof (dleq.go:57-79) and of share/pvss VerifyDecShare (pvss.go:250-266), one lane per element.  Each point is
 * hashed through the bytes MarshalTo writes for it (y reduced below p; the sign bit cleared where x = 0, i.e. y = 1 or
 * p - 1), computed from the wire bytes without a square root -- exact for every encoding that decodes; an encoding
 * that does not decode is the caller's to reject (the reference's UnmarshalBinary would have).  The suite's XOF is
 * BLAKE2Xb keyed with the 32-byte digest (suite.go:31, xof/blake2xb/blake.go:19-41); Pick reads 32 bytes big-endian,
 * masks them to 253 bits and redraws until the value is below l (scalar.go:180-184, util/random/rand.go:19-46).  c: n x 32
 * bytes little-endian.  status (may be NULL): 0, or KYB_ST_PICK_EXHAUSTED (c[i] zero) after 128 draws.
 * _dev: device pointers, 16-byte aligned. */
int kyb_ed25519_dleq_challenge(size_t n, const uint8_t *xG, const uint8_t *xH, const uint8_t *vG, const uint8_t *vH,
                               uint8_t *c, uint8_t *status);
int kyb_ed25519_dleq_challenge_dev(size_t n, const void *d_xG, const void *d_xH, const void *d_vG, const void *d_vH,
                                   void *d_c, void *d_status, void *stream);

/* ok[i] = 1 iff Proof{C[i], R[i], VG[i], VH[i]}.Verify(suite, G[i], H[i], xG[i], xH[i]) == nil: proof/dleq Proof.Verify
 * (dleq.go:160-172), both equations of a proof in one lane program -- a = r G + c xG and b = r H + c xH as two
 * Straus-Shamir chains over the same two table slots, r and c recoded once -- and the verdict encode(a) == VG &&
 * encode(b) == VH taken on bytes in the shared-inversion encode pass: Point.Equal on re-encodings (point.go:81-96).  VG
 * and VH are never decompressed; they are compared through their canonical bytes (see kyb_ed25519_dleq_challenge).
 * g_stride, h_stride: 32 for per-element bases, 0 for one 32-byte base shared by the batch (share/pvss shares H in
 * VerifyEncShare, pvss.go:154-163, and G in VerifyDecShare, pvss.go:248-276).
 * expect_c: NULL, or ONE 32-byte scalar every C[i] must equal -- the global challenge of pvss.go:154-157.
 * flags: 0 or a combination of KYB_F_VARTIME (the value semantics of kyb_ed25519_mul2's) and KYB_F_DLEQ_FS (C[i] must
 * equal the challenge derived on the device, pvss.go:250-270).  KYB_F_UNIFORM, any other bit, a stride that is neither
 * 0 nor 32, or KYB_F_DLEQ_FS together with expect_c is KYB_E_ARG before any device work.  Challenges are compared on
 * their raw 32 bytes, as scalar.Equal does on what UnmarshalBinary copied unreduced (scalar.go:37-45, 226-232): c + l is
 * another challenge.
 * status[i] (may be NULL), the reference's order as precedence: KYB_ST_PICK_EXHAUSTED, KYB_ST_DLEQ_CHALLENGE, then
 * KYB_ST_BAD_POINT if G, H, xG or xH does not decode; ok[i] is 0 with each.  Otherwise 0 and ok[i] carries the
 * equations' verdict; a VG or VH that is not a curve point lands there with ok = 0 (it can equal no point's encoding),
 * as an undecodable R does in kyb_ed25519_verify.  _dev: device pointers, 16-byte aligned. */
int kyb_ed25519_dleq_verify(size_t n, const uint8_t *G, size_t g_stride, const uint8_t *H, size_t h_stride,
                            const uint8_t *xG, const uint8_t *xH, const uint8_t *C, const uint8_t *R,
                            const uint8_t *VG, const uint8_t *VH, const uint8_t *expect_c,
                            uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_ed25519_dleq_verify_dev(size_t n, const void *d_G, size_t g_stride, const void *d_H, size_t h_stride,
                                const void *d_xG, const void *d_xH, const void *d_C, const void *d_R,
                                const void *d_VG, const void *d_VH, const void *d_expect_c,
                                void *d_ok, void *d_status, uint32_t flags, void *stream);

/* out[i] = the i-th scalar that n sequential Scalar.Pick calls return when they read ONE BLAKE2Xb stream from byte
 * position pos: the challenges hashProver.PubRand / hashVerifier.PubRand read into a []kyber.Scalar (hash.go:68-75,
 * hash.go:111-142), and the private draws of PriRand when the suite's random stream is that XOF.  root: the 64-byte
 * root hash of blake2b.NewXOF(OutputLengthUnknown, key) after its writes (blake.go:19-41) -- for the reseeded pool of
 * consumeMsg, the XOF keyed with 128 bytes of the old one (blake.go:55-74) after Write(transcript).  A draw is 32 stream
 * bytes read big-endian, the first masked to 253 bits, accepted iff below l (rand.go:19-46, scalar.go:180-184); pos is
 * any byte position, so a draw may straddle two output nodes.  draws_used: 32-byte draws consumed up to and including
 * the n-th accepted one; the caller advances its stream by 32 * draws_used.
 * The reference's loop is sequential; here every candidate draw of a fixed window of W(n) = 2n + 16 ceil(sqrt n) + 256
 * draws is tested by a lane of its own and the accepted ones are compacted in order (count, scan, scatter: three
 * launches, no workgroup waits on another).  The n-th accepted draw lies outside the window with the probability of an
 * eleven-sigma event; then the host variant returns KYB_E_EXHAUSTED (kyb_last_error names the call) and the _dev
 * variant writes 0 to d_draws_used and zeroes out.  KYB_E_ARG before any device work: a NULL pointer, n above 2^31, a
 * window that would pass output node 2^32 - 1 (the node offset is 32 bits).  n = 0 is KYB_OK and touches no device; the
 * host variant sets *draws_used = 0.  _dev: device pointers, out 16-byte and root, draws_used 8-byte aligned. */
int kyb_ed25519_xof_pick(size_t n, const uint8_t root[64], uint64_t pos, uint8_t *out, uint64_t *draws_used);
int kyb_ed25519_xof_pick_dev(size_t n, const void *d_root, uint64_t pos, void *d_out, void *d_draws_used, void *stream);

/* ok[i] = 1 iff encode(a[i] * (A[i] + U) + Neg(b[i]) * (B[i] + W)) equals the canonical bytes of T[i]: thver of the
 * simple k-shuffle (simple.go:178-183) over Xhat = X + U, Yhat = Y + W (simple.go:225-242), one lane per element -- two
 * window tables, one Straus-Shamir chain, the verdict taken on bytes in the shared-inversion encode pass.  The checks
 * of the pair shuffle with batch-wide bases (pair.go:295-309) stay on the fixed-base calls.
 * a, b, A, B, T: n x 32 bytes.  U, W: each NULL (nothing added) or ONE 32-byte point shared by the batch.
 * a[i] is used as its 32 wire bytes, never reduced, with kyb_ed25519_mul2's value under flags (0 or KYB_F_VARTIME;
 * KYB_F_UNIFORM or any other bit is KYB_E_ARG).  Neg(b) is scSub(0, b) (scalar.go:119-128): the reduced residue of -b
 * mod l, multiplied as a scalar -- not a negation of the point b * (B + W), which differs where B + W has a torsion
 * component.  T[i] is never decompressed: it is compared through its canonical bytes (see kyb_ed25519_dleq_challenge),
 * so a T that is no curve point gives ok = 0 with status 0.  status[i] (may be NULL) is KYB_ST_BAD_POINT, with ok[i] = 0,
 * if A[i], B[i], U or W does not decode, else 0.  _dev: device pointers, 16-byte aligned. */
int kyb_ed25519_theta_check(size_t n, const uint8_t *a, const uint8_t *A, const uint8_t *U, const uint8_t *b,
                            const uint8_t *B, const uint8_t *W, const uint8_t *T, uint8_t *ok, uint8_t *status,
                            uint32_t flags);
int kyb_ed25519_theta_check_dev(size_t n, const void *d_a, const void *d_A, const void *d_U, const void *d_b,
                                const void *d_B, const void *d_W, const void *d_T, void *d_ok, void *d_status,
                                uint32_t flags, void *stream);

/* out[i] = sum_{j < ko} s[i][j] * own[i][j] + sum_{j < ks} s[i][ko + j] * shared[j]: the linear combination of a Rep
 * predicate of proof/proof.go, one lane per element -- the commitment V = w P + v_1 B_1 + ... + v_k B_k
 * (proof.go:203-237) and the check V == c P + r_1 B_1 + ... + r_k B_k (proof.go:298-322).  ONE Straus-Shamir chain: one
 * chain of doublings, ko + ks additions per window, one encoding.  The points a batch shares (the predicate's bases)
 * are decoded and their window tables built once per call.
 * scalars: n x (ko + ks) x 32 bytes, element-major, own terms first.  own: n x ko x 32 bytes, NULL iff ko == 0.
 * shared: ks x 32 bytes, NULL iff ks == 0.  1 <= ko + ks, ko <= 4, ks <= 4.
 * Every term has the value kyb_ed25519_mul gives it under flags (0 or KYB_F_VARTIME), unreduced scalars and the
 * >= 2^255 behaviour included, as in kyb_ed25519_mul2.  Bit j of nil_mask makes shared term j Mul(s, nil): the standard
 * base with the value of kyb_ed25519_mul_base WITHOUT flags whatever flags says (point.go:243: Mul(s, nil) takes
 * geScalarMultBase; biffle_test.go:41 passes G = nil), as s G has in kyb_ed25519_ring_chain; the term's 32 bytes of
 * `shared` are not read.
 * expect: NULL, or n x 32 bytes; ok[i] = 1 iff the encoding equals the canonical bytes of expect[i], which is never
 * decompressed (see kyb_ed25519_theta_check): an expect[i] that is no curve point gives ok = 0 with status 0.  The
 * verdict is taken in the shared-inversion encode pass.  out: NULL, or n x 32 bytes.
 * status[i] (may be NULL) is KYB_ST_BAD_POINT if an own point of element i or any shared point that is used (not nil)
 * does not decode; out[i] is then zero bytes and ok[i] = 0.
 * KYB_E_ARG before any device work: KYB_F_UNIFORM or any other flag bit; nil_mask bits at or above ks; expect without
 * ok or ok without expect; out and ok both NULL; an own or shared pointer that contradicts ko or ks; ko or ks out of
 * range.  n = 0 is KYB_OK and touches no device.  The call runs on the current device: it is not sharded over a device
 * set.  _dev: device pointers, 16-byte aligned. */
int kyb_ed25519_lincomb(size_t n, size_t ko, size_t ks, const uint8_t *scalars, const uint8_t *own,
                        const uint8_t *shared, uint32_t nil_mask, const uint8_t *expect, uint8_t *out, uint8_t *ok,
                        uint8_t *status, uint32_t flags);
int kyb_ed25519_lincomb_dev(size_t n, size_t ko, size_t ks, const void *d_scalars, const void *d_own,
                            const void *d_shared, uint32_t nil_mask, const void *d_expect, void *d_out, void *d_ok,
                            void *d_status, uint32_t flags, void *stream);

/* c[i] = Scalar.Pick(X) with X = blake2xb.New(name_i), X.Reseed(), X.Write(data[i]): the one challenge of a hash-based
 * proof, what hashVerifier.PubRand draws after the prover's messages (hash.go:111-142 over blake.go:19-41, 55-74), one
 * lane per proof.  Reseed reads 128 stream bytes; the new XOF is keyed with the first 64 and the other 64, then
 * data[i], are written to it.  data_len = 0 means nothing was consumed: no reseed, the pick comes from New(name_i)
 * itself (hash.go:46-65).  A name longer than 64 bytes keys with its first 64 and writes the rest, as New does; an
 * empty name is a keyless root.
 * names: name i is names[name_off[i] .. name_off[i + 1]), n + 1 offsets as in kyb_ed25519_verify; with name_off NULL
 * every proof has the one name of name_len bytes (name_len is not read otherwise).  data: n x data_len bytes, data_len
 * a multiple of 32 (anything else is KYB_E_ARG).  c: n x 32 bytes little-endian.  status (may be NULL): 0, or
 * KYB_ST_PICK_EXHAUSTED (c[i] zero) after 128 draws, as in kyb_ed25519_dleq_challenge.  Decreasing offsets (host
 * variant) and a NULL names where offsets or a length name bytes are KYB_E_ARG.  n = 0 is KYB_OK and touches no device.
 * The call runs on the current device.  _dev: device pointers; name_off 8-byte and c 16-byte aligned, names and data of
 * any alignment; a pair of offsets that decreases is read as an empty name. */
int kyb_ed25519_fs_challenge(size_t n, const uint8_t *names, const uint64_t *name_off, size_t name_len,
                             const uint8_t *data, size_t data_len, uint8_t *c, uint8_t *status);
int kyb_ed25519_fs_challenge_dev(size_t n, const void *d_names, const void *d_name_off, size_t name_len,
                                 const void *d_data, size_t data_len, void *d_c, void *d_status, void *stream);

/* sign/cosi: n participation masks, or n collective signatures, over ONE roster of m public keys.
 *
 * kyb_ed25519_mask_aggregate: out[i] = the aggregate public key of mask i, count[i] = its enabled keys: Mask.SetMask,
 * Mask.AggregatePublic and Mask.CountEnabled (cosi.go:300-317, 361-372), where the reference makes up to m sequential
 * Point.Add calls per mask.  The roster is decoded once per call and cut into groups of 4 or 8 keys with a table of
 * every subset's sum; a mask then costs one addition per group, and a mask with more than half of its keys enabled is
 * taken through its complement, so full participation costs none.
 *   Let L = (m + 7) >> 3.  Element i's mask is the L bytes at masks + i * mask_stride, read byte by byte: no alignment
 *   is assumed, mask_stride >= L is required, and nothing beyond the last element's L bytes is read.  Bit j & 7 of
 *   byte j >> 3 enables roster key j.  Bits at or above m in the last byte are ignored, as the reference's loop over
 *   publics ignores them, in out and in count alike.  out[i] is the canonical encoding of the sum of the enabled keys;
 *   an empty mask gives the identity, 01 00 .. 00.  count (n words) and status (n bytes) may be NULL.
 *   Roster keys decode by the reference's rules: y >= p is reduced, "-0" is accepted, small-order points are points
 *   like any other.  If any roster key has no x, every status[i] is KYB_ST_BAD_POINT, every out[i] (agg[i]) is zero
 *   bytes and every ok[i] is 0 -- the rule of kyb_ed25519_mul_same_base.  count is the mask's own and is written anyway.
 *
 * kyb_ed25519_cosi_verify: ok[i] = 1 iff cosi.Verify's equation holds for signature i under mask i (cosi.go:214-232):
 * status[i] is 0 and canon(V_i) == encode((r_i mod l) B - k_i A_i) with k_i = SHA-512(V_i || encode(A_i) || msg_i) mod l.
 * sigs: n x 64 bytes, V || r (the mask that follows them in the reference's signature goes in masks); message i is
 * msgs[msg_off[i] .. msg_off[i + 1]), n + 1 offsets as in kyb_ed25519_verify.  The hash takes V's bytes as they stand
 * in the signature and A's canonical bytes.  r is reduced, not rejected: r + l verifies as r does.  Unlike
 * kyb_ed25519_verify there are no canonicity or small-order checks: the reference has none here.  V is compared
 * through its canonical bytes (y reduced, "-0" as 0) and never decompressed: a V that is no curve point equals no
 * point's encoding, so ok = 0 with status 0.  agg (n x 32), count and status may be NULL.  The participation policy
 * (sign/policy.go) is the caller's, over count.
 *
 * Both: flags must be 0; 1 <= m <= KYB_COSI_MAX_ROSTER; a NULL roster, masks, out or ok (sigs, msg_off) with n > 0, a
 * stride below L, a non-zero flag and -- host variant -- decreasing message offsets are KYB_E_ARG, decided before any
 * device is touched.  n = 0 is KYB_OK and touches nothing; nothing is written past element n - 1.  The calls run on
 * the current device and do not consult the device set; the tables are per call: (m + 7) / 8 * 256 * 160 bytes at the
 * widest, 42 MB for 8192 keys.  Addresses follow the masks, which are public.  _dev: device pointers, enqueued on
 * `stream`; roster, sigs and agg 16-byte aligned, count 4-byte, msg_off 8-byte, masks and msgs of any alignment; a pair
 * of offsets that decreases is read as an empty message.
 * kyb_ed25519_cosi_group_width: the table width, 4 or 8, a call of this shape uses (no device is touched). */
#define KYB_COSI_MAX_ROSTER 8192
int kyb_ed25519_mask_aggregate(size_t n, size_t m, const uint8_t *roster /* m x 32 */, const uint8_t *masks,
                               size_t mask_stride, uint8_t *out /* n x 32 */, uint32_t *count, uint8_t *status,
                               uint32_t flags);
int kyb_ed25519_mask_aggregate_dev(size_t n, size_t m, const void *d_roster, const void *d_masks, size_t mask_stride,
                                   void *d_out, void *d_count, void *d_status, uint32_t flags, void *stream);
int kyb_ed25519_cosi_verify(size_t n, size_t m, const uint8_t *roster, const uint8_t *msgs, const uint64_t *msg_off,
                            const uint8_t *sigs /* n x 64: V || r */, const uint8_t *masks, size_t mask_stride,
                            uint8_t *agg, uint32_t *count, uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_ed25519_cosi_verify_dev(size_t n, size_t m, const void *d_roster, const void *d_msgs, const void *d_msg_off,
                                const void *d_sigs, const void *d_masks, size_t mask_stride, void *d_agg, void *d_count,
                                void *d_ok, void *d_status, uint32_t flags, void *stream);
int kyb_ed25519_cosi_group_width(size_t n, size_t m);

/* encrypt/ecies Encrypt (ecies.go:23-69) for a batch, hash = SHA-256.  r: n x 32 ephemeral scalars, drawn by the caller
 * (Pick(random.New()) in the reference).  pubs: n x 32 bytes (pub_stride = 32) or ONE recipient of every message
 * (pub_stride = 0).  Message i is msgs[msg_off[i] .. msg_off[i + 1]), n + 1 offsets, as in kyb_ed25519_verify.
 * Ciphertext i, msg length + 48 bytes, is written at out + msg_off[i] + 48 i: R = r B (32 bytes, kyb_ed25519_mul_base's
 * at flags 0), then AES-256-GCM.Seal(key, nonce, msg, no additional data) -- the ciphertext and its 16-byte tag -- with
 * key || nonce the first 44 bytes of HKDF-SHA256(secret = the 32 bytes of r pub (kyb_ed25519_mul's at flags 0), salt =
 * nil, info = nil) (ecies.go:115-127).  status[i] (may be NULL) is KYB_ST_BAD_POINT, with an all-zero slot, where pub
 * does not decode (kyb_ed25519_unmarshal's rule).  Decreasing offsets or a stride that is neither 0 nor 32 are KYB_E_ARG
 * before any device work; n = 0 is KYB_OK and touches nothing.  _dev: device pointers, r, pubs and msg_off 16-byte
 * aligned; offsets are the caller's contract, a decreasing pair is read as an empty element. */
int kyb_ed25519_ecies_seal(size_t n, const uint8_t *r, const uint8_t *pubs, size_t pub_stride, const uint8_t *msgs,
                           const uint64_t *msg_off, uint8_t *out, uint8_t *status);
int kyb_ed25519_ecies_seal_dev(size_t n, const void *d_r, const void *d_pubs, size_t pub_stride, const void *d_msgs,
                               const void *d_msg_off, void *d_out, void *d_status, void *stream);
/* encrypt/ecies Decrypt (ecies.go:77-112).  privs: n x 32 bytes (priv_stride = 32) or ONE receiver of n ciphertexts
 * (priv_stride = 0, the DKG's case); the scalar is used as kyb_ed25519_mul uses it at flags 0.  Element i is
 * ctx[ctx_off[i] .. ctx_off[i + 1]); its plaintext (48 bytes shorter) is written at out + ctx_off[i], zero bytes behind
 * it up to out + ctx_off[i + 1]: out is as large as ctx.  status[i] (may be NULL), the reference's order as precedence:
 * KYB_ST_ECIES_SHORT (fewer than 48 bytes; nothing of the element is read), KYB_ST_BAD_POINT (R does not decode),
 * KYB_ST_ECIES_AUTH (tag mismatch).  The slot of an element with a non-zero status is all zero bytes: unauthenticated
 * plaintext never leaves the device.  Argument errors, n = 0 and _dev as for kyb_ed25519_ecies_seal. */
int kyb_ed25519_ecies_open(size_t n, const uint8_t *privs, size_t priv_stride, const uint8_t *ctx, const uint64_t *ctx_off,
                           uint8_t *out, uint8_t *status);
int kyb_ed25519_ecies_open_dev(size_t n, const void *d_privs, size_t priv_stride, const void *d_ctx, const void *d_ctx_off,
                               void *d_out, void *d_status, void *stream);

/* ok[i] = Equal(Mul(shares[i], nil), NewPubPoly(.., commits of polynomial poly[i]).Eval(idx[i]).V): the share check of
 * share/dkg's ProcessDeals and ProcessJustifications (dkg.go:488-495, 824-832; share/poly.go:340-348, 405-409 with the
 * standard base), many polynomials at one or a few indices each.  commits: m polynomials of t encoded points
 * (m t x 32 bytes); check i names polynomial poly[i], the index idx[i] (evaluated at x = idx[i] + 1) and a 32-byte
 * share.  The left side has kyb_ed25519_mul_base's value at flags 0 for every 32-byte scalar (never reduced,
 * scalar.go:226-232); the right side equals kyb_ed25519_poly_eval of that polynomial at that index; t = 0 evaluates to
 * the identity.  status (may be NULL) has m entries: status[k] is KYB_ST_BAD_POINT if any commitment of polynomial k
 * does not decode, every check that names k then has ok = 0, and the other polynomials are unaffected.  poly[i] >= m:
 * KYB_E_ARG before any device work from the host variant; ok[i] = 0 with nothing read for that check from the _dev
 * variant.  m t commitments the workspace cannot hold are KYB_E_ALLOC.  n = 0 is KYB_OK and touches nothing (status
 * included).  _dev: device pointers, 16-byte aligned. */
int kyb_ed25519_deal_check(size_t n, const uint32_t *poly, const uint32_t *idx, const uint8_t *shares, size_t m, size_t t,
                           const uint8_t *commits, uint8_t *ok, uint8_t *status);
int kyb_ed25519_deal_check_dev(size_t n, const void *d_poly, const void *d_idx, const void *d_shares, size_t m, size_t t,
                               const void *d_commits, void *d_ok, void *d_status, void *stream);

/* sign/schnorr Sign (schnorr.go:56-82) for a batch.  k: n x 32 nonces, drawn by the caller (the reference picks them from
 * the suite's stream).  privs: n x 32 bytes (priv_stride = 32) or ONE signer of every message (priv_stride = 0).  Message i
 * is msgs[msg_off[i] .. msg_off[i + 1]), n + 1 offsets, as in kyb_ed25519_verify.  sigs: n x 64 bytes R || S with R = k B
 * and A = x B (kyb_ed25519_mul_base's values at flags 0, both encodings from one shared inversion),
 * h = SHA-512(R || A || msg) mod l and S = k + h x mod l; k and x may be any 32 bytes.  A signature made here passes
 * kyb_ed25519_verify under A.  status (may be NULL) is written 0: nothing can fail per element.  A stride that is neither
 * 0 nor 32, a NULL pointer with n > 0 or -- host variant -- decreasing offsets are KYB_E_ARG before any device work; n = 0
 * is KYB_OK and touches nothing.  Runs on the current device.  _dev: device pointers, k, privs, sigs and msg_off 16-byte
 * aligned; a decreasing pair of offsets is read as an empty message. */
int kyb_ed25519_schnorr_sign(size_t n, const uint8_t *k, const uint8_t *privs, size_t priv_stride, const uint8_t *msgs,
                             const uint64_t *msg_off, uint8_t *sigs, uint8_t *status);
int kyb_ed25519_schnorr_sign_dev(size_t n, const void *d_k, const void *d_privs, size_t priv_stride, const void *d_msgs,
                                 const void *d_msg_off, void *d_sigs, void *d_status, void *stream);

/* share/vss Dealer.EncryptedDeal (pedersen/vss.go:222-255; rabin/vss.go:263-297 with ctx_len = 128) for the n verifiers
 * of one dealer.
 * dh, k: n x 32 ephemeral scalars and signature nonces, drawn by the caller.  Element i gives
 *   dhkeys[i]  = dh_i B (32 bytes);
 *   sigs[i]    = schnorr.Sign(dealer_priv, dhkeys[i]) under the nonce k_i (64 bytes), with dealer_pub -- the caller's
 *                contract: dealer_priv B -- hashed as the public key;
 *   cipher i   = AES-256-GCM.Seal(key, nonce = 12 zero bytes, msg_i, additional data = ctx), msg length + 16 bytes, at
 *                ciphers + msg_off[i] + 16 i, with key the first 32 bytes of HKDF-SHA256(secret = the 32 bytes of
 *                dh_i pubs_i (kyb_ed25519_mul's at flags 0), salt = nil, info = ctx) (dh.go:23-40).
 * ctx: ctx_len bytes -- 32, pedersen's SHA-256 context (dh.go:43-51), or 128, rabin's XOF context (rabin/dh.go:42-66) --
 * one for the batch (ctx_stride = 0) or one per element (ctx_stride = ctx_len); any other length or stride is KYB_E_ARG.
 * The info of the HKDF is ctx (one expand step either way), the additional data two or eight blocks.  status[i] (may be NULL) is
 * KYB_ST_BAD_POINT, with all three outputs of the element zero, where pubs_i does not decode.  Offsets, n = 0, argument
 * errors and the alignment rules of _dev follow kyb_ed25519_ecies_seal (dh, k, the two dealer keys, pubs, ctx, dhkeys
 * and sigs 16-byte aligned).  Runs on the current device. */
int kyb_ed25519_vss_seal(size_t n, const uint8_t *dh, const uint8_t *k, const uint8_t *dealer_priv /* 32 */,
                         const uint8_t *dealer_pub /* 32 */, const uint8_t *pubs, const uint8_t *ctx, size_t ctx_stride,
                         size_t ctx_len, const uint8_t *msgs, const uint64_t *msg_off, uint8_t *dhkeys, uint8_t *sigs,
                         uint8_t *ciphers, uint8_t *status);
int kyb_ed25519_vss_seal_dev(size_t n, const void *d_dh, const void *d_k, const void *d_dealer_priv, const void *d_dealer_pub,
                             const void *d_pubs, const void *d_ctx, size_t ctx_stride, size_t ctx_len, const void *d_msgs,
                             const void *d_msg_off, void *d_dhkeys, void *d_sigs, void *d_ciphers, void *d_status, void *stream);
/* The second half of share/vss decryptDeal (pedersen/vss.go:443-457, rabin/vss.go:490-503): pre = x DHKey, the same key derivation, then Open
 * under the zero nonce with ctx as additional data.  The signature over DHKey (vss.go:439) is kyb_ed25519_verify's,
 * called first by the caller.  privs: n x 32 bytes or ONE receiver (priv_stride = 0); dhkeys: n x 32; cipher i is
 * ciphers[ct_off[i] .. ct_off[i + 1]); its plaintext (16 bytes shorter) is written at out + ct_off[i], zero bytes behind
 * it.  status[i] (may be NULL), in this precedence: KYB_ST_ECIES_SHORT (fewer than 16 bytes), KYB_ST_BAD_POINT (DHKey does
 * not decode), KYB_ST_ECIES_AUTH; the slot of such an element is all zero: the tag is checked before a plaintext byte
 * leaves the device.  Everything else as for kyb_ed25519_ecies_open. */
int kyb_ed25519_vss_open(size_t n, const uint8_t *privs, size_t priv_stride, const uint8_t *dhkeys, const uint8_t *ctx,
                         size_t ctx_stride, size_t ctx_len, const uint8_t *ciphers, const uint64_t *ct_off, uint8_t *out, uint8_t *status);
int kyb_ed25519_vss_open_dev(size_t n, const void *d_privs, size_t priv_stride, const void *d_dhkeys, const void *d_ctx,
                             size_t ctx_stride, size_t ctx_len, const void *d_ciphers, const void *d_ct_off, void *d_out, void *d_status,
                             void *stream);

/* Rabin's VerifyDeal equation (rabin/vss.go:611-651): ok[i] = Equal(Add(Mul(f_i, nil), Mul(g_i, H_k)),
 * PubPoly(commits of polynomial k).Eval(idx[i]).V) with k = poly[i].  Everything kyb_ed25519_deal_check documents holds:
 * raw 32-byte scalars, never reduced; x = idx + 1; t = 0; poly[i] >= m; status per polynomial; no inversion.  Mul(g, H)
 * has kyb_ed25519_mul's value at flags 0 for every 32-byte g and every H that decodes, points with a torsion component
 * and the identity included.  H: one point for the batch (h_stride = 0) or one per polynomial (h_stride = 32); an H that
 * does not decode marks its polynomial -- every polynomial, at h_stride = 0 -- KYB_ST_BAD_POINT, as a bad commitment
 * does.  H is decoded and its window table built once per polynomial; the checks read it from global memory. */
int kyb_ed25519_deal_check2(size_t n, const uint32_t *poly, const uint32_t *idx, const uint8_t *f_shares,
                            const uint8_t *g_shares, size_t m, size_t t, const uint8_t *commits, const uint8_t *H,
                            size_t h_stride, uint8_t *ok, uint8_t *status);
int kyb_ed25519_deal_check2_dev(size_t n, const void *d_poly, const void *d_idx, const void *d_f, const void *d_g, size_t m,
                                size_t t, const void *d_commits, const void *d_H, size_t h_stride, void *d_ok, void *d_status,
                                void *stream);

/* sign/dss ProcessPartialSig (dss.go:141-173) without its sequential state: n partial signatures spread over ns sessions
 * of ONE long-term key and ONE roster.  participants: np x 32 key bytes; long_commits: tl x 32, the long-term key's
 * commitments; rand_commits: ns x tr x 32, each session's random key; message b is msgs[msg_off[b] .. msg_off[b + 1]),
 * ns + 1 offsets, as in kyb_ed25519_verify.  Partial i names the session sess[i] and the signer idx[i] and carries V[i]
 * (32 bytes), its session id sid[i] (32 bytes) and sig[i] (64 bytes).
 * Per session b (dss.go:201-211, 235-246): h_b = SHA-512(rand_commits[b][0] || long_commits[0] || msg_b) mod l, sid_b =
 * SHA-256(long_commits || rand_commits[b]) -- the commitments enter through the bytes given, as MarshalTo writes them --
 * and the folded commitments D_{b,k} = R_{b,k} + h_b A_k, k < max(tl, tr), a missing term being the identity.  A session
 * with a commitment that does not decode gets sess_status[b] = KYB_ST_BAD_POINT (the long-term key's: every session) and
 * every partial that names it ok = 0; other sessions are unaffected.
 * Per partial, the reference's order as the status precedence:
 *   KYB_ST_DSS_INDEX     idx[i] >= np; nothing else of the element is read            ErrInvalidSignatureIndex
 *   the signature        schnorr.VerifyWithChecks(participants[idx], m, sig) over m = SHA-256(SHA-256(V || u32le(idx)) ||
 *                        sid): kyb_ed25519_verify's ok and status for the same (key, m, sig) -- KYB_ST_SIG_NONCANONICAL,
 *                        KYB_ST_SIG_SMALL_ORDER, KYB_ST_BAD_POINT as they stand -- and KYB_ST_DSS_SIG where only the
 *                        equation fails
 *   KYB_ST_DSS_SESSION   sid[i] != sid_b                                              "dss: session id do not match"
 *   KYB_ST_BAD_POINT     the session's commitments do not decode (no counterpart: the reference holds decoded points)
 *   KYB_ST_DSS_PARTIAL   V B != sum_k D_{b,k} (idx + 1)^k                             "dss: partial signature not valid"
 * V B has kyb_ed25519_mul_base's value at flags 0 for every 32 bytes of V (never reduced); the verdict is projective, as
 * in kyb_ed25519_deal_check, and exact for every input: sum_k x^k D_{b,k} = randomPoly.Eval(I).V + h longPoly.Eval(I).V
 * on the whole curve group.  The duplicate rule ("already received from peer", dss.go:156-158) is sequential state and the
 * caller's, between KYB_ST_DSS_SESSION and KYB_ST_DSS_PARTIAL.  ok[i] = 1 only with status 0.  status and sess_status may
 * be NULL.  n = 0 is KYB_OK and touches nothing; with n > 0 a NULL required pointer, tl = 0, tr = 0 (the hash needs
 * commitment 0), ns = 0 or -- host variant -- decreasing offsets are KYB_E_ARG before any device work.  sess[i] >= ns:
 * KYB_E_ARG from the host variant; ok[i] = 0 (status 0) with nothing read for that partial from the _dev variant.
 * ns max(tl, tr) commitments the workspace cannot hold are KYB_E_ALLOC.  Runs on the current device.  _dev: device
 * pointers, all but msgs 16-byte aligned; a decreasing pair of offsets is read as an empty message. */
int kyb_ed25519_dss_check(size_t n, size_t np, const uint8_t *participants, size_t tl, const uint8_t *long_commits, size_t ns,
                          size_t tr, const uint8_t *rand_commits, const uint8_t *msgs, const uint64_t *msg_off,
                          const uint32_t *sess, const uint32_t *idx, const uint8_t *V, const uint8_t *sid, const uint8_t *sigs,
                          uint8_t *ok, uint8_t *status, uint8_t *sess_status);
int kyb_ed25519_dss_check_dev(size_t n, size_t np, const void *d_participants, size_t tl, const void *d_long_commits, size_t ns,
                              size_t tr, const void *d_rand_commits, const void *d_msgs, const void *d_msg_off, const void *d_sess,
                              const void *d_idx, const void *d_V, const void *d_sid, const void *d_sigs, void *d_ok, void *d_status,
                              void *d_sess_status, void *stream);
/* sign/dss PartialSig (dss.go:113-134) for ns sessions of one signer.  priv: the signer's long-term secret (32 bytes), index
 * its position in the roster; alpha: its share of the long-term key (32 bytes); beta: ns x 32, its shares of the sessions'
 * random keys; k: ns x 32 Schnorr nonces, drawn by the caller as kyb_ed25519_schnorr_sign's are; commitments and messages
 * as in kyb_ed25519_dss_check.  Session b gives V[b] = h_b alpha + beta_b mod l (32 bytes), sid[b] (32 bytes) and
 * sig[b] = schnorr.Sign(priv, SHA-256(SHA-256(V[b] || u32le(index)) || sid[b])) under the nonce k_b (64 bytes): the bytes of
 * kyb_ed25519_schnorr_sign on the same nonce and message.  A = priv B is computed once per call; every point comes from
 * the comb through the shared-inversion encoder.  Nothing can fail per element.  ns = 0 is KYB_OK and touches nothing; a
 * NULL pointer, tl = 0, tr = 0 or -- host variant -- decreasing offsets are KYB_E_ARG; ns max(tl, tr) above 2^31 is
 * KYB_E_ALLOC from both variants, as in kyb_ed25519_dss_check.  Runs on the current device.
 * _dev: device pointers, all but msgs 16-byte aligned. */
int kyb_ed25519_dss_partial(size_t ns, const uint8_t *priv /* 32 */, uint32_t index, const uint8_t *alpha /* 32 */,
                            const uint8_t *beta, const uint8_t *k, size_t tl, const uint8_t *long_commits, size_t tr,
                            const uint8_t *rand_commits, const uint8_t *msgs, const uint64_t *msg_off, uint8_t *V, uint8_t *sid,
                            uint8_t *sigs);
int kyb_ed25519_dss_partial_dev(size_t ns, const void *d_priv, uint32_t index, const void *d_alpha, const void *d_beta,
                                const void *d_k, size_t tl, const void *d_long_commits, size_t tr, const void *d_rand_commits,
                                const void *d_msgs, const void *d_msg_off, void *d_V, void *d_sid, void *d_sigs, void *stream);

/* sign/eddsa key expansion for a batch of seeds: Curve.NewKeyAndSeedWithInput (group/edwards25519/curve.go:51-60) followed
 * by Mul(secret, nil) (eddsa.go:50-51, 81-86).  seeds: n x 32 bytes.  With digest = SHA-512(seed), secrets[i] (32 bytes) is
 * digest[0:32] after &= 0xf8 on byte 0 and &= 0x7f, |= 0x40 on byte 31, stored UNREDUCED as the reference stores it;
 * prefixes[i] (32 bytes) is digest[32:64]; pubs[i] (32 bytes) is the canonical encoding of secret B, byte for byte
 * kyb_ed25519_mul_base's at flags 0 (the hash and the comb in one lane, the encodings from one shared inversion).  Nothing
 * can fail per element.  A NULL pointer with n > 0 is KYB_E_ARG before any device work; n = 0 is KYB_OK and touches
 * nothing.  Runs on the current device.  _dev: device pointers, 16-byte aligned. */
int kyb_ed25519_eddsa_expand(size_t n, const uint8_t *seeds, uint8_t *secrets, uint8_t *prefixes, uint8_t *pubs);
int kyb_ed25519_eddsa_expand_dev(size_t n, const void *d_seeds, void *d_secrets, void *d_prefixes, void *d_pubs, void *stream);
/* sign/eddsa (*EdDSA).Sign (eddsa.go:91-142) for a batch.  secrets, prefixes, pubs: a key's three parts as
 * kyb_ed25519_eddsa_expand gives them, n x 32 bytes each (key_stride = 32) or ONE key signing every message (key_stride =
 * 0); one stride governs all three.  Message i is msgs[msg_off[i] .. msg_off[i + 1]), n + 1 offsets, as in
 * kyb_ed25519_verify.  sigs: n x 64 bytes R || S with r = SHA-512(prefix || msg) mod l, R = r B (kyb_ed25519_mul_base's
 * value at flags 0), h = SHA-512(R || pub || msg) mod l and S = r + h secret mod l; secret may be any 32 bytes.  pubs is
 * hashed as its bytes stand (eddsa.go:110-118): it is neither decoded nor recomputed, so a signature verifies under pub
 * only when pub is secret B.  status (may be NULL) is written 0: nothing can fail per element.  A stride that is neither 0
 * nor 32, a NULL pointer with n > 0 or -- host variant -- decreasing offsets are KYB_E_ARG before any device work; n = 0 is
 * KYB_OK and touches nothing.  Runs on the current device.  _dev: device pointers, secrets, prefixes, pubs, sigs and
 * msg_off 16-byte aligned; a decreasing pair of offsets is read as an empty message. */
int kyb_ed25519_eddsa_sign(size_t n, const uint8_t *secrets, const uint8_t *prefixes, const uint8_t *pubs, size_t key_stride,
                           const uint8_t *msgs, const uint64_t *msg_off, uint8_t *sigs, uint8_t *status);
int kyb_ed25519_eddsa_sign_dev(size_t n, const void *d_secrets, const void *d_prefixes, const void *d_pubs, size_t key_stride,
                               const void *d_msgs, const void *d_msg_off, void *d_sigs, void *d_status, void *stream);

/* sign/anon Encrypt (enc.go:123-148 over encryptKey and header(), enc.go:11-40) for a batch.  keys: the anonymity set,
 * ring x 32 bytes shared by the batch (key_stride = 0) or one set per message (key_stride = 32 ring), 1 <= ring <=
 * KYB_ANON_MAX_RING.  x: n x 32 ephemeral private keys, drawn by the caller (key.Pair.Gen: the suite's NewKey, clamped and
 * UNREDUCED, curve.go:51-76); the products use them as kyb_ed25519_mul uses a scalar at flags 0, and the device derives
 * the master secret xb = x mod l (Private.MarshalBinary) itself.  Message i is msgs[msg_off[i] .. msg_off[i + 1]), n + 1
 * offsets, as in kyb_ed25519_ecies_seal.  Ciphertext i, 48 + 32 ring bytes longer than its message, is written at
 * out + msg_off[i] + i (48 + 32 ring):  X = x B (kyb_ed25519_mul_base's at flags 0) || ring slots || ctx || mac  with
 * slot k = xb ^ BLAKE2Xb(key = the 32 bytes of x keys[k])[0:32], ctx = msg ^ BLAKE2Xb(key = xb) and mac =
 * BLAKE2Xb(ctx)[0:16], the first <= 64 bytes of ctx being the hash's key (blake.go:19-41).  status[i] (may be NULL) is
 * KYB_ST_BAD_POINT, with an all-zero slot, where a ring member of that message does not decode (kyb_ed25519_unmarshal's
 * rule).  KYB_E_ARG before any device work: ring = 0 or above KYB_ANON_MAX_RING, a key_stride that is neither 0 nor
 * 32 ring, a NULL pointer with n > 0, decreasing offsets (host variant); n = 0 is KYB_OK and touches nothing.  Runs on the
 * current device.  _dev: device pointers, keys, x and msg_off 16-byte aligned (msgs and out: any alignment); offsets are
 * the caller's contract, a decreasing pair is read as an empty message. */
int kyb_ed25519_anon_seal(size_t n, size_t ring, const uint8_t *keys, size_t key_stride, const uint8_t *x, const uint8_t *msgs,
                          const uint64_t *msg_off, uint8_t *out, uint8_t *status);
int kyb_ed25519_anon_seal_dev(size_t n, size_t ring, const void *d_keys, size_t key_stride, const void *d_x, const void *d_msgs,
                              const void *d_msg_off, void *d_out, void *d_status, void *stream);
/* sign/anon Decrypt (enc.go:165-192 over decryptKey, enc.go:44-102).  keys and key_stride as above; mine: n uint32, the
 * receiver's position in the set of element i; privs: n x 32 bytes (priv_stride = 32) or ONE receiver of every ciphertext
 * (priv_stride = 0), used as kyb_ed25519_mul uses a scalar at flags 0.  Element i is ctx[ctx_off[i] .. ctx_off[i + 1]);
 * its plaintext (48 + 32 ring bytes shorter) is written at out + ctx_off[i], zero bytes behind it up to
 * out + ctx_off[i + 1]: out is as large as ctx.  The 32 bytes recovered from slot mine are the scalar of x B and of the
 * regenerated header as they are, never reduced (scalar.go:226-232), so a set with a member outside the prime-order
 * subgroup is rejected here though Encrypt sealed for it, as in the reference; the raw first 32 bytes go back into that
 * header, so an X that decodes is not rejected for a non-canonical encoding alone.
 * status[i] (may be NULL), the reference's order of checks as precedence:
 *   KYB_ST_ANON_SHORT    fewer than 32 bytes (nothing of the element is read)          "ciphertext too short"
 *   KYB_ST_BAD_POINT     X does not decode                                             X.UnmarshalBinary's error
 *   KYB_ST_ANON_SHORT    fewer than 32 + 32 ring bytes                                 "ciphertext too short"
 *   KYB_ST_BAD_POINT     a ring member does not decode (the reference's Set holds decoded points: no counterpart)
 *   KYB_ST_ANON_INVALID  x B != X on canonical bytes, or a slot of the regenerated header differs: EVERY member's slot
 *                        is recomputed, which is what keeps a sender from de-anonymising a receiver   "invalid ciphertext"
 *   KYB_ST_ANON_SHORT    fewer than 32 + 32 ring + 16 bytes                            "ciphertext too short"
 *   KYB_ST_ANON_MAC      the MAC differs                                  "invalid ciphertext: failed MAC check"
 * The slot of an element with a non-zero status is all zero bytes: the MAC is decided before a plaintext byte is written.
 * KYB_E_ARG as for kyb_ed25519_anon_seal, and for a priv_stride that is neither 0 nor 32; in the host variant also for
 * mine[i] >= ring (the reference panics), which the _dev variant takes modulo ring.  _dev: device pointers, keys, mine,
 * privs and ctx_off 16-byte aligned (ctx and out: any alignment). */
int kyb_ed25519_anon_open(size_t n, size_t ring, const uint8_t *keys, size_t key_stride, const uint32_t *mine, const uint8_t *privs,
                          size_t priv_stride, const uint8_t *ctx, const uint64_t *ctx_off, uint8_t *out, uint8_t *status);
int kyb_ed25519_anon_open_dev(size_t n, size_t ring, const void *d_keys, size_t key_stride, const void *d_mine, const void *d_privs,
                              size_t priv_stride, const void *d_ctx, const void *d_ctx_off, void *d_out, void *d_status, void *stream);

/* The ring loop of sign/anon (Rivest ring signatures and Liu-Wei-Wong linkable ring signatures), one lane per
 * signature running its whole hash chain: Verify's loop (sig.go:231-238) with start = NULL and steps = ring, and the
 * open ring of Sign (sig.go:159-166) with start[i] = mine + 1 and steps = ring - 1.  Position p computes
 * PG = s_p G + c X_p and, for a linkable signature, PH = s_p linkBase + c tag, and the next challenge
 * c = Scalar.Pick(suite.XOF(msg) after Write(scope), Write(tag), Write(PG), Write(PH)) (signH1 over signH1pre,
 * sig.go:23-43): BLAKE2Xb keyed with the first <= 64 message bytes, the rest written as data (blake.go:19-41).
 * keys: the anonymity set, ring x 32 bytes shared by the batch (key_stride = 0) or one set per signature
 * (key_stride = 32 ring).  Message i is msgs[msg_off[i] .. msg_off[i + 1]), as in kyb_ed25519_verify.
 * scope: NULL for unlinkable signatures, otherwise scope_len >= 0 bytes (a non-NULL pointer even when empty) and
 * link_base, the 32 bytes of Point.Pick(suite.XOF(scope)) (sig.go:131-132), which the caller derives once.
 * sigs: the wire layout c_0 || s_0 .. s_{ring-1} || [tag], sig_stride = 32 (ring + 1) or 32 (ring + 2) bytes apart.
 * Scalars are the wire bytes, never reduced.  s G has the value of kyb_ed25519_mul_base without flags whatever `flags`
 * says (Mul(s, nil) is geScalarMultBase, point.go:243); the other products have kyb_ed25519_mul's value under `flags`,
 * 0 or KYB_F_VARTIME, with the meaning it has in kyb_ed25519_mul2.  The tag is hashed through the bytes MarshalBinary
 * writes for it (see kyb_ed25519_dleq_challenge).
 * Lane i starts at position start[i] (NULL: 0 for all; host variant: start[i] >= ring is KYB_E_ARG, _dev: taken modulo
 * ring) with the challenge in slot 0 of sigs[i] and runs `steps` positions, wrapping modulo ring.  c_out[i]: the last
 * challenge; with steps = 0 no position runs, c_out[i] is slot 0 itself and ok[i] = 1 whatever the signature says: a
 * verifier passes steps = ring.  c_zero[i]: the challenge that entered position 0 -- the input challenge when start[i] = 0, zero bytes
 * if position ring - 1 was never run.  ok[i] = (status[i] == 0 && c_out[i] == slot 0 of sigs[i], on bytes:
 * scalar.Equal, sig.go:238).  status[i]: KYB_ST_PICK_EXHAUSTED, else KYB_ST_BAD_POINT when link_base, the tag or a
 * ring member the chain visited does not decode; c_zero[i] and c_out[i] are then zero bytes.  c_zero, c_out, ok and
 * status may each be NULL.
 * KYB_E_ARG before any device work: ring = 0, a key_stride or sig_stride other than the values above, a link_base
 * without a scope or a scope without one, any flag but KYB_F_VARTIME (KYB_F_UNIFORM included).  n = 0 is KYB_OK and
 * touches no device.  _dev: device pointers, 16-byte aligned (msgs and scope: any alignment). */
int kyb_ed25519_ring_chain(size_t n, size_t ring, const uint8_t *keys, size_t key_stride,
                           const uint8_t *msgs, const uint64_t *msg_off, const uint8_t *scope, size_t scope_len,
                           const uint8_t *link_base, const uint8_t *sigs, size_t sig_stride,
                           const uint32_t *start, size_t steps,
                           uint8_t *c_zero, uint8_t *c_out, uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_ed25519_ring_chain_dev(size_t n, size_t ring, const void *d_keys, size_t key_stride,
                               const void *d_msgs, const void *d_msg_off, const void *d_scope, size_t scope_len,
                               const void *d_link_base, const void *d_sigs, size_t sig_stride,
                               const void *d_start, size_t steps,
                               void *d_c_zero, void *d_c_out, void *d_ok, void *d_status, uint32_t flags, void *stream);

/* c[i] = signH1(signH1pre(msgs[i], scope, tags[i]), PG[i], PH[i]): the hash step of sign/anon alone (sig.go:34-43 over
 * sig.go:23-32), one lane per element -- the first challenge of Sign (sig.go:152), the counterpart of
 * kyb_ed25519_dleq_challenge.  scope, tags and PH are NULL for unlinkable signatures (a tag or a PH without a scope is
 * KYB_E_ARG).  tags[i] is hashed through its canonical bytes; PG[i] and PH[i] are hashed as given (they are what
 * MarshalBinary wrote).  status (may be NULL): 0, or KYB_ST_PICK_EXHAUSTED (c[i] zero).  _dev: device pointers, tags,
 * PG, PH and c 16-byte aligned. */
int kyb_ed25519_ring_challenge(size_t n, const uint8_t *msgs, const uint64_t *msg_off,
                               const uint8_t *scope, size_t scope_len, const uint8_t *tags,
                               const uint8_t *PG, const uint8_t *PH, uint8_t *c, uint8_t *status);
int kyb_ed25519_ring_challenge_dev(size_t n, const void *d_msgs, const void *d_msg_off,
                                   const void *d_scope, size_t scope_len, const void *d_tags,
                                   const void *d_PG, const void *d_PH, void *d_c, void *d_status, void *stream);

/* out[i] = MarshalBinary(UnmarshalBinary(points[i])), status[i] = the error UnmarshalBinary would return:
 * (*point).UnmarshalBinary (group/edwards25519/point.go:65-70 -> ge.go:110-150; bit 255 of y is only the sign of x,
 * y >= p is accepted, no subgroup check) followed by MarshalBinary (point.go:54-58), i.e. the canonical encoding.
 * Rejected slots give 32 zero bytes. */
int kyb_ed25519_unmarshal(size_t n, const uint8_t *points, uint8_t *out, uint8_t *status);
int kyb_ed25519_unmarshal_dev(size_t n, const void *d_points, void *d_out, void *d_status, void *stream);

/* out[i] = Hash(msgs[i], dst): (*point).Hash (group/edwards25519/point.go:325-334), RFC 9380 suite
 * edwards25519_XMD:SHA-512_ELL2_RO_ (hashToField :336-360, expandMessageXMD :362-430, Elligator 2, cofactor 8).
 * Equal-length messages packed back to back; dst is a HOST pointer of 1..255 bytes. */
int kyb_ed25519_hash(size_t n, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, uint8_t *out);
int kyb_ed25519_hash_dev(size_t n, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len,
                         void *d_out, void *stream);

/* Introspection used by the tests: copy the device-built fixed-base table
 * (33 x 8 entries of (y+x, y-x, 2dxy), 10 int32 limbs each) to the host. */
int kyb_ed25519_debug_base_table(int32_t *out /* 33*136*32: (position, |digit|-1, 30 limbs + 2 pad) */);

/* The standard base's wide comb (built at init, used by the fixed-base batches without KYB_F_UNIFORM):
 * info = {digits per position G, positions, rows per position, rows of the last position, bytes, build time in us};
 * debug_comb_table copies rows row0 .. row0+nrows-1 of one position, 32 int32 each (30 limbs + 2 pad), row j holding
 * (j+1) * 16^(G*pos) * B as (y+x, y-x, 2dxy). */
int kyb_ed25519_comb_info(int64_t info[6]);
int kyb_ed25519_debug_comb_table(int pos, int row0, int nrows, int32_t *out);

/* --------------------------------------------------------------- BLS12-381
 * The three reference suites pairing/bls12381/{kilic,circl,gnark} are adapters over external
 * modules (go.mod:6-8); their MarshalBinary wire formats are identical and are what crosses
 * this boundary:
 *   scalars : 32-byte big-endian (mod.Int, group/mod/int.go:334-350; kilic/scalar.go), taken as
 *             plain 256-bit integers
 *   G1      : 48-byte ZCash compressed (kilic/g1.go:119-131)      G2 : 96-byte (kilic/g2.go)
 *   GT      : 576 bytes (kilic/gt.go:115-117); layout documented in DESIGN.md (parity unpinned
 *             by the reference)
 * UnmarshalBinary semantics: flag rules + on-curve + subgroup membership, exactly the cases of
 * pairing/bls12381/deserialization_tests (bls12381_test.go:74-186).  A rejected input gives
 * status KYB_ST_BAD_POINT / KYB_ST_NOT_IN_SUBGROUP and an all-zero output element.          */

/* out[i] = scalars[i] * points[i].  Replaces G1Elt.UnmarshalBinary + Mul + MarshalBinary
 * (pairing/bls12381/kilic/g1.go:110-131; circl/g1.go:89-96; gnark/g1.go:118-127). */
int kyb_bls12381_g1_mul(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
/* same on G2 (kilic/g2.go; this is what suite.Point().Mul is for the *.adapter suites) */
int kyb_bls12381_g2_mul(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
/* out[i] = scalars[i] * point: the loop of share.PriPoly.Commit (share/poly.go:143-149).  Batches of 2^17 scalars and
 * more -- and, through the host-buffer calls, batches of 64 and more over the suite's generator or over the base of
 * the previous call -- run through a table of the base's multiples (26 table additions per scalar, no doublings; same
 * bytes and statuses as the per-element calls; the same holds for the bn256 / bn254 entry points and for the `_dev`
 * calls with point_stride = 0). */
int kyb_bls12381_g1_mul_same_base(size_t n, const uint8_t *scalars, const uint8_t point[48], uint8_t *out,
                                  uint8_t *status, uint32_t flags);
int kyb_bls12381_g2_mul_same_base(size_t n, const uint8_t *scalars, const uint8_t point[96], uint8_t *out,
                                  uint8_t *status, uint32_t flags);
/* point_stride: the input element size (48 / 96, or 96 / 192 with KYB_F_UNCOMPRESSED) for per-element points,
 * 0 for one shared base point */
int kyb_bls12381_g1_mul_dev(size_t n, const void *d_scalars, const void *d_points, size_t point_stride, void *d_out,
                            void *d_status, uint32_t flags, void *stream);
int kyb_bls12381_g2_mul_dev(size_t n, const void *d_scalars, const void *d_points, size_t point_stride, void *d_out,
                            void *d_status, uint32_t flags, void *stream);

/* out[i] = a[i] + b[i]: G1Elt.Add / G2Elt.Add (kilic/g1.go:90-96, g2.go).  Both operands are decoded under every rule
 * of UnmarshalBinary, the subgroup included, whatever the other one gave.  status[i] is a[i]'s status if that is not
 * KYB_ST_OK, else b[i]'s (an operand off the subgroup next to a malformed one: the status of the one in slot a), and
 * out[i] is zero bytes unless both are KYB_ST_OK; a sum at infinity is the canonical 0xC0 00 .. 00.  status (d_status)
 * may be NULL: the outputs are the same, zero bytes on the rejected elements included.  Nothing is written past
 * element n - 1; n = 0 is KYB_OK; a NULL a, b or out with n > 0 is KYB_E_ARG. */
int kyb_bls12381_g1_add(size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *status);
int kyb_bls12381_g2_add(size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *status);
/* the same on device pointers, enqueued on `stream` (kilic/g1.go:90-96): what the node-wide MSM's combine of the gathered partial
 * points uses, so that nothing of the exchange step touches the host */
int kyb_bls12381_g1_add_dev(size_t n, const void *d_a, const void *d_b, void *d_out, void *d_status, void *stream);
int kyb_bls12381_g2_add_dev(size_t n, const void *d_a, const void *d_b, void *d_out, void *d_status, void *stream);

/* Batch UnmarshalBinary: status[i] = what G1Elt / G2Elt.UnmarshalBinary would decide (kilic/g1.go:127-131, g2.go:
 * ZCash flag rules, x < p, on the curve, in the r-torsion subgroup -- the 34 fixtures of
 * pairing/bls12381/deserialization_tests), out[i] = the point re-encoded (48 / 96 B, or 96 / 192 B affine with
 * KYB_F_UNCOMPRESSED_OUT; zero bytes when rejected).  Input is compressed unless KYB_F_UNCOMPRESSED.  This is the
 * call that earns KYB_F_TRUSTED(i) | KYB_F_UNCOMPRESSED on later calls with the same points. */
int kyb_bls12381_g1_unmarshal(size_t n, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bls12381_g2_unmarshal(size_t n, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bls12381_g1_unmarshal_dev(size_t n, const void *d_points, void *d_out, void *d_status, uint32_t flags, void *stream);
int kyb_bls12381_g2_unmarshal_dev(size_t n, const void *d_points, void *d_out, void *d_status, uint32_t flags, void *stream);

/* gt[i] = e(g1[i], g2[i]).  Replaces Suite.Pair (pairing/pairing.go:12; kilic/suite.go:70-75). */
int kyb_bls12381_pair(size_t n, const uint8_t *g1, const uint8_t *g2, uint8_t *gt, uint8_t *status, uint32_t flags);
int kyb_bls12381_pair_dev(size_t n, const void *d_g1, const void *d_g2, void *d_gt, void *d_status, uint32_t flags, void *stream);
/* out[i] = hash_to_curve(msgs[i], dst) on G1 / G2 (RFC 9380 BLS12381G1/G2_XMD:SHA-256_SSWU_RO_).  Replaces
 * G1Elt.Hash / G2Elt.Hash (pairing/bls12381/kilic/g1.go:161-170, g2.go; default DSTs kilic/g1.go:17, g2.go:18), the
 * step before the pairing check in sign/bls Verify (bls.go:87-88).  The n messages have the same length msg_len
 * and are packed back to back; dst is a HOST pointer (at most 255 bytes) in every variant. */
int kyb_bls12381_hash_g1(size_t n, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len,
                         uint8_t *out, uint8_t *status);
int kyb_bls12381_hash_g2(size_t n, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len,
                         uint8_t *out, uint8_t *status);
int kyb_bls12381_hash_g1_dev(size_t n, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len,
                             void *d_out, void *d_status, void *stream);
int kyb_bls12381_hash_g2_dev(size_t n, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len,
                             void *d_out, void *d_status, void *stream);
/* ok[i] = bls.Verify(pubkeys[i], msgs[i], sigs[i]) for the scheme with signatures on G1 and keys on G2
 * (sign/bls/bls.go:82-96 with the pairing closure of bls.go:36-38): e(H(msg), X) == e(sig, G2.Base()), hashing,
 * both UnmarshalBinary checks, two Miller loops and one final exponentiation fused per lane (the hashed point is
 * never encoded / re-decoded).  Equal-length messages packed back to back; dst is a HOST pointer.  status[i] != 0
 * (and ok[i] = 0) where the key or the signature does not unmarshal -- the reference returns an error there. */
int kyb_bls12381_verify_g1(size_t n, const uint8_t *pubkeys, const uint8_t *msgs, size_t msg_len, const uint8_t *dst,
                           size_t dst_len, const uint8_t *sigs, uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_bls12381_verify_g1_dev(size_t n, const void *d_pubkeys, const void *d_msgs, size_t msg_len,
                               const uint8_t *dst, size_t dst_len, const void *d_sigs, void *d_ok, void *d_status,
                               uint32_t flags, void *stream);
/* ok[i] = bls.Verify(pubkey, msgs[i], sigs[i]) for ONE public key (96 B, or 192 B with KYB_F_UNCOMPRESSED; a HOST
 * pointer in the first variant, a device pointer in `_dev`): sign/bls/bls.go:82-96 called in a loop with the same X --
 * a drand chain's beacons, the partial signatures of one tbls participant (sign/tbls/tbls.go:100-107).  With both G2
 * operands the same for every element, both Miller loops read their lines from tables (the generator's is a constant of
 * the program; the key's is built on the device the first time a key is seen and kept with those of the last eight keys
 * of the stream -- looked up on the device -- so that a verifier alternating between a few keys pays the walk once per key).  The key is checked as UnmarshalBinary would (KYB_F_TRUSTED(0) vouches for it);
 * a key that fails gives every element its status and ok = 0; status precedence per element: key, then signature. */
int kyb_bls12381_verify_g1_same_key(size_t n, const uint8_t *pubkey, const uint8_t *msgs, size_t msg_len,
                                    const uint8_t *dst, size_t dst_len, const uint8_t *sigs, uint8_t *ok,
                                    uint8_t *status, uint32_t flags);
int kyb_bls12381_verify_g1_same_key_dev(size_t n, const void *d_pubkey, const void *d_msgs, size_t msg_len,
                                        const uint8_t *dst, size_t dst_len, const void *d_sigs, void *d_ok,
                                        void *d_status, uint32_t flags, void *stream);
/* test hook: out3 = {cache hits, table builds, next slot} of `stream`'s key cache behind kyb_bls12381_verify_g1_same_key
 * (sign/bls/bls.go:82-96 over a committee of keys); synchronises the stream */
int kyb_bls12381_debug_vkey_stats(void *stream, uint32_t *out3);
/* ok[i] = bls.Verify(pubkeys[i], msg, sigs[i]) for ONE message: the verification loop of tbls.Recover
 * (sign/tbls/tbls.go:118-131 -- every partial signature of a round is over the same msg, each under its own public
 * share public.Eval(idx).V, share/poly.go:340-348).  H(msg) is computed once per call instead of once per element;
 * everything else is kyb_bls12381_verify_g1 (same flags, same status precedence: key, then signature).  `msg` is a HOST
 * pointer in the first variant, a device pointer in `_dev`; msg_len may be 0. */
int kyb_bls12381_verify_g1_same_msg(size_t n, const uint8_t *pubkeys, const uint8_t *msg, size_t msg_len,
                                    const uint8_t *dst, size_t dst_len, const uint8_t *sigs, uint8_t *ok,
                                    uint8_t *status, uint32_t flags);
int kyb_bls12381_verify_g1_same_msg_dev(size_t n, const void *d_pubkeys, const void *d_msg, size_t msg_len,
                                        const uint8_t *dst, size_t dst_len, const void *d_sigs, void *d_ok,
                                        void *d_status, uint32_t flags, void *stream);
/* The same for the scheme with signatures on G2 and keys on G1 (NewSchemeOnG2, sign/bls/bls.go:48-58:
 * ValidatePairing(G1.Base(), sig, X, H(msg)) with H = hash_to_curve on G2): pubkeys 48 B, sigs 96 B. */
int kyb_bls12381_verify_g2(size_t n, const uint8_t *pubkeys, const uint8_t *msgs, size_t msg_len, const uint8_t *dst,
                           size_t dst_len, const uint8_t *sigs, uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_bls12381_verify_g2_dev(size_t n, const void *d_pubkeys, const void *d_msgs, size_t msg_len,
                               const uint8_t *dst, size_t dst_len, const void *d_sigs, void *d_ok, void *d_status,
                               uint32_t flags, void *stream);
/* out[i] = gt[i] ^ scalars[i].  Replaces GTElt.Mul (kilic/gt.go:79-84 -> GT.Exp); inputs are checked
 * like GT.FromBytes (coefficients < p, order-r subgroup). */
int kyb_bls12381_gt_mul(size_t n, const uint8_t *scalars, const uint8_t *gt, uint8_t *out, uint8_t *status);
int kyb_bls12381_gt_mul_dev(size_t n, const void *d_scalars, const void *d_gt, void *d_out, void *d_status,
                            void *stream);
/* encrypt/ibe, the Boneh-Franklin CCA scheme (ibe.go:51-232) with the suite hash SHA-256 and the 576-byte GT bytes of
 * kyb_bls12381_pair, one ciphertext (U, V, W) per element:
 *   _g1: EncryptCCAonG1 / DecryptCCAonG1 (ibe.go:51-135): master key and U on G1, identity and private key on G2
 *        (drand's "chained" / "unchained" networks);
 *   _g2: EncryptCCAonG2 / DecryptCCAonG2 (ibe.go:137-232): master key and U on G2, identity and private key on G1
 *        (drand quicknet).
 * Every element of a call has the same message length msg_len, 0..32 (more is KYB_E_ARG: the reference's "plaintext /
 * ciphertext too long"); V and W are msg_len bytes each, packed back to back.
 *
 * Encrypt: Gid = e(master, H(id)) (_g2: e(H(id), master); H = hash_to_curve under `dst`, a HOST pointer) once per call, then
 * per element r = h3(sigma, msg) (ibe.go:234-281), U = r Base, V = sigma ^ H2(Gid^r), W = msg ^ H4(sigma).  The sigmas
 * (msg_len bytes each) are the caller's: the reference draws them from crypto/rand (ibe.go:61-65); taking them as input
 * keeps the engine deterministic.  U is written compressed, or uncompressed with KYB_F_UNCOMPRESSED_OUT.
 * KYB_F_TRUSTED(0) vouches for the master key, KYB_F_UNCOMPRESSED makes it uncompressed.  status[i]: the master key's
 * UnmarshalBinary status, then KYB_ST_IBE_H3; U, V and W are zero bytes where it is not 0.
 *
 * Decrypt: msgs[i] = the plaintext, or zero bytes where status[i] != 0.  private_stride: 0 for ONE private key for every
 * element (a tlock round: one beacon opens every ciphertext locked to it), or the key's wire size (96 / 48 B, 192 / 96 B
 * with KYB_F_UNCOMPRESSED) for one key per element; anything else is KYB_E_ARG.  KYB_F_TRUSTED(0) vouches for the
 * private keys, KYB_F_TRUSTED(1) for the U points, KYB_F_UNCOMPRESSED makes both uncompressed.  Status precedence per
 * element: the key's UnmarshalBinary status, then U's, then KYB_ST_IBE_H3, then KYB_ST_IBE_CHECK (rP != U).
 * `_dev`: every buffer a device pointer (id and master included; dst stays a host pointer), enqueued on `stream`. */
int kyb_bls12381_ibe_encrypt_g1(size_t n, const uint8_t *master, const uint8_t *id, size_t id_len, const uint8_t *dst,
                                size_t dst_len, const uint8_t *sigmas, const uint8_t *msgs, size_t msg_len, uint8_t *u,
                                uint8_t *v, uint8_t *w, uint8_t *status, uint32_t flags);
int kyb_bls12381_ibe_encrypt_g2(size_t n, const uint8_t *master, const uint8_t *id, size_t id_len, const uint8_t *dst,
                                size_t dst_len, const uint8_t *sigmas, const uint8_t *msgs, size_t msg_len, uint8_t *u,
                                uint8_t *v, uint8_t *w, uint8_t *status, uint32_t flags);
int kyb_bls12381_ibe_decrypt_g1(size_t n, const uint8_t *privates, size_t private_stride, const uint8_t *u, const uint8_t *v,
                                const uint8_t *w, size_t msg_len, uint8_t *msgs, uint8_t *status, uint32_t flags);
int kyb_bls12381_ibe_decrypt_g2(size_t n, const uint8_t *privates, size_t private_stride, const uint8_t *u, const uint8_t *v,
                                const uint8_t *w, size_t msg_len, uint8_t *msgs, uint8_t *status, uint32_t flags);
int kyb_bls12381_ibe_encrypt_g1_dev(size_t n, const void *d_master, const void *d_id, size_t id_len, const uint8_t *dst,
                                    size_t dst_len, const void *d_sigmas, const void *d_msgs, size_t msg_len, void *d_u,
                                    void *d_v, void *d_w, void *d_status, uint32_t flags, void *stream);
int kyb_bls12381_ibe_encrypt_g2_dev(size_t n, const void *d_master, const void *d_id, size_t id_len, const uint8_t *dst,
                                    size_t dst_len, const void *d_sigmas, const void *d_msgs, size_t msg_len, void *d_u,
                                    void *d_v, void *d_w, void *d_status, uint32_t flags, void *stream);
int kyb_bls12381_ibe_decrypt_g1_dev(size_t n, const void *d_privates, size_t private_stride, const void *d_u, const void *d_v,
                                    const void *d_w, size_t msg_len, void *d_msgs, void *d_status, uint32_t flags, void *stream);
int kyb_bls12381_ibe_decrypt_g2_dev(size_t n, const void *d_privates, size_t private_stride, const void *d_u, const void *d_v,
                                    const void *d_w, size_t msg_len, void *d_msgs, void *d_status, uint32_t flags, void *stream);
/* ok[i] = (e(p1[i], p2[i]) == e(inv1[i], inv2[i])).  Replaces Suite.ValidatePairing
 * (pairing/pairing.go:13-15; kilic/suite.go:57-68), the core of sign/bls Verify (bls.go:82-96). */
int kyb_bls12381_pair_check(size_t n, const uint8_t *p1, const uint8_t *p2, const uint8_t *inv1, const uint8_t *inv2,
                            uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_bls12381_pair_check_dev(size_t n, const void *d_p1, const void *d_p2, const void *d_inv1, const void *d_inv2,
                                void *d_ok, void *d_status, uint32_t flags, void *stream);

/* ------------------------------------------------------------------ bn256
 * pairing/bn256 (dclxvi parameters; arithmetic in-tree).  Wire formats (point.go):
 *   scalars : 32-byte big-endian (mod.Int), taken as plain 256-bit integers (curve.go:189-203)
 *   G1      : 64 bytes x || y, big-endian, infinity = 64 zero bytes (point.go:170-238)
 *   G2      : 128 bytes x.x || x.y || y.x || y.y with gfP2{x, y} = x i + y (point.go:423-499)
 *   GT      : 384 bytes, 12 x 32, order x.x.x ... y.z.y (point.go:630-662)
 * UnmarshalBinary semantics kept: coordinates are reduced mod p (not rejected), (0,0) is
 * infinity, on-curve check only -- G2 inputs outside the order-n subgroup are accepted and
 * processed like the reference does.  status: KYB_ST_BAD_POINT, output zeroed.
 * flags: KYB_F_TRUSTED(i) on a G2 operand is the caller's word that the point lies in the order-n subgroup (which this
 * suite's UnmarshalBinary never checks): g2_mul then walks a GLS decomposition and pair_check (below) the product form;
 * a vouched-for point outside the subgroup gives a result the reference could not.  Otherwise flags have no effect. */
int kyb_bn256_g1_mul(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bn256_g2_mul(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bn256_g1_mul_same_base(size_t n, const uint8_t *scalars, const uint8_t point[64], uint8_t *out,
                               uint8_t *status, uint32_t flags);
int kyb_bn256_g2_mul_same_base(size_t n, const uint8_t *scalars, const uint8_t point[128], uint8_t *out,
                               uint8_t *status, uint32_t flags);
int kyb_bn256_g1_mul_dev(size_t n, const void *d_scalars, const void *d_points, size_t point_stride, void *d_out,
                         void *d_status, uint32_t flags, void *stream);
int kyb_bn256_g2_mul_dev(size_t n, const void *d_scalars, const void *d_points, size_t point_stride, void *d_out,
                         void *d_status, uint32_t flags, void *stream);
/* out[i] = a[i] + b[i]: pointG1.Add / pointG2.Add (pairing/bn256/point.go:130-140, 381-391 -> curve.go:69).  Operands
 * are decoded as UnmarshalBinary does (a coordinate >= p reduced, all-zero bytes = infinity, on the curve / twist); a G2
 * operand outside the order-n subgroup is a point of the twist and is added as one.  status[i] is a[i]'s status if
 * that is not KYB_ST_OK, else b[i]'s, and out[i] is zero bytes unless both are KYB_ST_OK -- which is also how a sum at
 * infinity reads, so status tells the two apart.  status (d_status) may be NULL: the outputs are the same.  Nothing is
 * written past element n - 1; n = 0 is KYB_OK; a NULL a, b or out with n > 0 is KYB_E_ARG. */
int kyb_bn256_g1_add(size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *status);
int kyb_bn256_g2_add(size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *status);
/* the same on device pointers, enqueued on `stream` (pairing/bn256/point.go:130-140): what the node-wide MSM's combine of the gathered partial
 * points uses, so that nothing of the exchange step touches the host */
int kyb_bn256_g1_add_dev(size_t n, const void *d_a, const void *d_b, void *d_out, void *d_status, void *stream);
int kyb_bn256_g2_add_dev(size_t n, const void *d_a, const void *d_b, void *d_out, void *d_status, void *stream);
/* Batch UnmarshalBinary: pointG1 / pointG2.UnmarshalBinary (pairing/bn256/point.go:206-238, 466-499): on the curve
 * (G2: on the twist, NO subgroup check, as the reference), 64 / 128 zero bytes = infinity; out[i] = MarshalBinary of
 * the accepted point (zero bytes when rejected).  flags are accepted and ignored. */
int kyb_bn256_g1_unmarshal(size_t n, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bn256_g2_unmarshal(size_t n, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bn256_g1_unmarshal_dev(size_t n, const void *d_points, void *d_out, void *d_status, uint32_t flags, void *stream);
int kyb_bn256_g2_unmarshal_dev(size_t n, const void *d_points, void *d_out, void *d_status, uint32_t flags, void *stream);

/* gt[i] = e(g1[i], g2[i]): Suite.Pair (pairing/bn256/suite.go:97-103 -> optate.go:266-274). */
int kyb_bn256_pair(size_t n, const uint8_t *g1, const uint8_t *g2, uint8_t *gt, uint8_t *status, uint32_t flags);
int kyb_bn256_pair_dev(size_t n, const void *d_g1, const void *d_g2, void *d_gt, void *d_status, uint32_t flags, void *stream);
/* out[i] = Hash(msgs[i]) on G1: pointG1.Hash -> hashToPoint (pairing/bn256/point.go:261-313), SHA-256 then
 * try-and-increment; the step before the pairing check in sign/bls Verify (bls.go:87-88).  All n messages
 * have the same length msg_len and are packed back to back (hash variable-length inputs down first). */
int kyb_bn256_hash_g1(size_t n, const uint8_t *msgs, size_t msg_len, uint8_t *out, uint8_t *status);
int kyb_bn256_hash_g1_dev(size_t n, const void *d_msgs, size_t msg_len, void *d_out, void *d_status, void *stream);
/* out[i] = HashG1(msgs[i], dst): the package-level hash of pairing/bn256/hash.go:10-110 -- hashToBase (gfp.go:46-68:
 * 48 bytes of HKDF-SHA-256 with secret = msg, salt = dst, info = "H2C" 0x00 0x01, reduced mod p) then the
 * Shallue-van de Woestijne map in the reference's arrangement (x1, x2, x3 tried in this order with legendre == 1,
 * y = the power (p + 1) / 4 with sign0(t)'s sign; s = sqrt(-3) of constants.go:105).  dst may be NULL / empty
 * (hash_test.go:11-20 passes nil), at most 255 bytes.  Pinned by the 11 outputs of hash_test.go:45-57. */
int kyb_bn256_hash_g1_svdw(size_t n, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, uint8_t *out,
                           uint8_t *status);
int kyb_bn256_hash_g1_svdw_dev(size_t n, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out,
                               void *d_status, void *stream);
/* out[i] = gt[i] ^ scalars[i]: pointGT.Mul (pairing/bn256/point.go:613-628 -> gfP12.Exp gfp12.go:177);
 * like pointGT.UnmarshalBinary (point.go:664-716) coefficients are reduced mod p and nothing is rejected. */
int kyb_bn256_gt_mul(size_t n, const uint8_t *scalars, const uint8_t *gt, uint8_t *out, uint8_t *status);
int kyb_bn256_gt_mul_dev(size_t n, const void *d_scalars, const void *d_gt, void *d_out, void *d_status, void *stream);
/* ok[i] = Pair(p1, p2).Equal(Pair(inv1, inv2)): Suite.ValidatePairing (suite.go:105-107): two whole pairings and a
 * comparison, like the reference.  With KYB_F_TRUSTED(1) | KYB_F_TRUSTED(3) -- the caller vouches that both G2
 * operands lie in the order-n subgroup, which bn256's own UnmarshalBinary never checks -- the same predicate is
 * evaluated as e(p1, p2) e(-inv1, inv2) == 1 with one final exponentiation (1.6x the rate). */
int kyb_bn256_pair_check(size_t n, const uint8_t *p1, const uint8_t *p2, const uint8_t *inv1, const uint8_t *inv2,
                         uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_bn256_pair_check_dev(size_t n, const void *d_p1, const void *d_p2, const void *d_inv1, const void *d_inv2,
                             void *d_ok, void *d_status, uint32_t flags, void *stream);

/* ------------------------------------------------------------------ bn254
 * pairing/bn254 (Ethereum's alt_bn128; the bn256 package over other constants, xi = 9 + i).  Wire formats and entry
 * points as bn256 (scalars 32-byte big-endian, G1 64, G2 128, GT 384 bytes; point.go:127-200, 431-520, 617-735), with
 * this suite's stricter UnmarshalBinary kept:
 *   - a coordinate >= p is an error (gfp.go:101-118), not reduced                      -> KYB_ST_BAD_POINT
 *   - G2 points must lie in the order-n subgroup (twist.go:47-66: [Order]Q = infinity)  -> KYB_ST_NOT_IN_SUBGROUP
 *     KYB_F_TRUSTED(i) on a G2 operand skips that check (the caller unmarshalled the point before), as on BLS12-381.
 *   - GT coefficients >= p are rejected by gt_mul (point.go:662-735).
 * pointG1.Mul walks a GLV lattice decomposition (curve.go:196-222); the multiple is the same group element.
 * ValidatePairing = two pairings + Equal (suite.go:134-140).  No Hash on G2 (the reference has none). */
int kyb_bn254_g1_mul(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bn254_g2_mul(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bn254_g1_mul_same_base(size_t n, const uint8_t *scalars, const uint8_t point[64], uint8_t *out,
                               uint8_t *status, uint32_t flags);
int kyb_bn254_g2_mul_same_base(size_t n, const uint8_t *scalars, const uint8_t point[128], uint8_t *out,
                               uint8_t *status, uint32_t flags);
int kyb_bn254_g1_mul_dev(size_t n, const void *d_scalars, const void *d_points, size_t point_stride, void *d_out,
                         void *d_status, uint32_t flags, void *stream);
int kyb_bn254_g2_mul_dev(size_t n, const void *d_scalars, const void *d_points, size_t point_stride, void *d_out,
                         void *d_status, uint32_t flags, void *stream);
/* out[i] = a[i] + b[i] as kyb_bn256_g*_add (status precedence, zero output, NULL status, argument errors), under
 * bn254's decoding: a coordinate >= p is KYB_ST_BAD_POINT.  G2 operands are NOT re-checked against the subgroup --
 * operands of Add are point objects, validated when they were unmarshalled -- so a twist point outside it is added as
 * a point of the twist, never KYB_ST_NOT_IN_SUBGROUP. */
int kyb_bn254_g1_add(size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *status);
int kyb_bn254_g2_add(size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *status);
/* the same on device pointers, enqueued on `stream` (pairing/bn254/point.go:92-101): what the node-wide MSM's combine of the gathered partial
 * points uses, so that nothing of the exchange step touches the host */
int kyb_bn254_g1_add_dev(size_t n, const void *d_a, const void *d_b, void *d_out, void *d_status, void *stream);
int kyb_bn254_g2_add_dev(size_t n, const void *d_a, const void *d_b, void *d_out, void *d_status, void *stream);
int kyb_bn254_g1_unmarshal(size_t n, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bn254_g2_unmarshal(size_t n, const uint8_t *points, uint8_t *out, uint8_t *status, uint32_t flags);
int kyb_bn254_g1_unmarshal_dev(size_t n, const void *d_points, void *d_out, void *d_status, uint32_t flags, void *stream);
int kyb_bn254_g2_unmarshal_dev(size_t n, const void *d_points, void *d_out, void *d_status, uint32_t flags, void *stream);
int kyb_bn254_pair(size_t n, const uint8_t *g1, const uint8_t *g2, uint8_t *gt, uint8_t *status, uint32_t flags);
int kyb_bn254_pair_dev(size_t n, const void *d_g1, const void *d_g2, void *d_gt, void *d_status, uint32_t flags, void *stream);
int kyb_bn254_gt_mul(size_t n, const uint8_t *scalars, const uint8_t *gt, uint8_t *out, uint8_t *status);
int kyb_bn254_gt_mul_dev(size_t n, const void *d_scalars, const void *d_gt, void *d_out, void *d_status, void *stream);
int kyb_bn254_pair_check(size_t n, const uint8_t *p1, const uint8_t *p2, const uint8_t *inv1, const uint8_t *inv2,
                         uint8_t *ok, uint8_t *status, uint32_t flags);
int kyb_bn254_pair_check_dev(size_t n, const void *d_p1, const void *d_p2, const void *d_inv1, const void *d_inv2,
                             void *d_ok, void *d_status, uint32_t flags, void *stream);
/* out[i] = Hash(msgs[i]) on G1: pointG1.Hash -> hashToPoint (point.go:207-285): RFC 9380 hash_to_curve with
 * expand_message_xmd over legacy Keccak-256, the Shallue-van de Woestijne map (constants.go:72-84), no cofactor.
 * dst = the suite's domain separation tag (suite.go:42-44: "BN254G1_XMD:KECCAK-256_SVDW_RO_" unless SetDomainG1), at
 * most 255 bytes.  All n messages have the same length msg_len and are packed back to back. */
int kyb_bn254_hash_g1(size_t n, const uint8_t *msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, uint8_t *out,
                      uint8_t *status);
int kyb_bn254_hash_g1_dev(size_t n, const void *d_msgs, size_t msg_len, const uint8_t *dst, size_t dst_len, void *d_out,
                          void *d_status, void *stream);

/* ------------------------------------------------------- multi-scalar multiplication
 * out = sum_i scalars[i] * points[i]  (one point).  The reference has no MSM function: its
 * MSM-shaped call sites do N x (Mul + Add) sequentially -- share.PubPoly.Eval (share/poly.go:340-348),
 * share.RecoverCommit (share/poly.go:449-476), bdn.AggregateSignatures / AggregatePublicKeys
 * (sign/bdn/bdn.go:126-181, mask.go:57-61).  Encodings are canonical, so the Pippenger result is
 * byte-identical to that sequential sum -- for every 32-byte scalar: an Ed25519 scalar that the
 * reference's radix-16 recoding mangles (top digit above 8, see kyb_ed25519_mul) counts as the integer
 * the reference's Mul multiplies by.  status[i] reports undecodable inputs; if any input is
 * rejected the output is all-zero bytes.  n == 0 yields the encoding of the identity.
 * The _dev variants work in a grow-only workspace per (device, stream).                            */
int kyb_ed25519_msm(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t out[32], uint8_t *status);
/* the same with flags (KYB_F_SCALAR_BITS) */
int kyb_ed25519_msm_flags(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t out[32], uint8_t *status,
                          uint32_t flags);
int kyb_ed25519_msm_dev(size_t n, const void *d_scalars, const void *d_points, void *d_out, void *d_status,
                        void *stream);
int kyb_bls12381_g1_msm(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t out[48], uint8_t *status, uint32_t flags);
int kyb_bls12381_g2_msm(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t out[96], uint8_t *status, uint32_t flags);
int kyb_bls12381_g1_msm_dev(size_t n, const void *d_scalars, const void *d_points, void *d_out, void *d_status,
                            uint32_t flags, void *stream);
int kyb_bls12381_g2_msm_dev(size_t n, const void *d_scalars, const void *d_points, void *d_out, void *d_status,
                            uint32_t flags, void *stream);
int kyb_bn256_g1_msm(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t out[64], uint8_t *status, uint32_t flags);
int kyb_bn256_g2_msm(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t out[128], uint8_t *status, uint32_t flags);
int kyb_bn256_g1_msm_dev(size_t n, const void *d_scalars, const void *d_points, void *d_out, void *d_status,
                         uint32_t flags, void *stream);
int kyb_bn256_g2_msm_dev(size_t n, const void *d_scalars, const void *d_points, void *d_out, void *d_status,
                         uint32_t flags, void *stream);

/* --------------------------------------------------------- batched public-polynomial evaluation
 * out[i] = sum_j commits[j] * (idx[i] + 1)^j  (n points).  share.PubPoly.Eval (share/poly.go:340-348: xi = 1 + i,
 * Horner from the top coefficient with t x (Mul + Add)) for many indices in one launch -- the per-participant loop of
 * PubPoly.Shares / Check and of the DKG / VSS share verification (share/dkg/pedersen/dkg.go:294, 489-490, 825-826).
 * commits: t encoded points (coefficient 0 first); status[j] reports an undecodable commitment, and then every
 * output is all-zero bytes.  t == 0 yields identities.  flags as for the MSM (KYB_F_TRUSTED(0) = the commitments).  */
int kyb_ed25519_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *commits, uint8_t *out,
                          uint8_t *status);
int kyb_ed25519_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_commits, void *d_out,
                              void *d_status, void *stream);
int kyb_bls12381_g1_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *commits, uint8_t *out,
                              uint8_t *status, uint32_t flags);
int kyb_bls12381_g2_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *commits, uint8_t *out,
                              uint8_t *status, uint32_t flags);
int kyb_bls12381_g1_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_commits, void *d_out,
                                  void *d_status, uint32_t flags, void *stream);
int kyb_bls12381_g2_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_commits, void *d_out,
                                  void *d_status, uint32_t flags, void *stream);
int kyb_bn256_g1_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *commits, uint8_t *out,
                           uint8_t *status, uint32_t flags);
int kyb_bn256_g2_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *commits, uint8_t *out,
                           uint8_t *status, uint32_t flags);
int kyb_bn256_g1_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_commits, void *d_out,
                               void *d_status, uint32_t flags, void *stream);
int kyb_bn256_g2_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_commits, void *d_out,
                               void *d_status, uint32_t flags, void *stream);
/* --------------------------------------------------------- batched private-polynomial evaluation (scalar field)
 * out[i] = sum_j coeffs[j] * (idx[i] + 1)^j mod q  (n scalars of 32 bytes, q = the group order).  share.PriPoly.Eval
 * (share/poly.go:85-93: xi = 1 + i, Horner from the top coefficient with t x (Mul + Add) of group/mod.Int) for many
 * indices in one launch -- the loop of PriPoly.Shares (share/poly.go:96-102), which every dealer of share/vss and
 * share/dkg runs once per participant.  coeffs: t scalars in the suite's scalar encoding (Ed25519: 32 bytes
 * little-endian, group/edwards25519/scalar.go; pairing suites: mod.Int's 32 bytes big-endian, group/mod/int.go);
 * any 32-byte string is taken modulo q; outputs are canonical.  t == 0 yields zeros.                              */
int kyb_ed25519_scalar_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *coeffs, uint8_t *out);
int kyb_ed25519_scalar_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_coeffs, void *d_out, void *stream);
int kyb_bls12381_scalar_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *coeffs, uint8_t *out);
int kyb_bls12381_scalar_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_coeffs, void *d_out, void *stream);
int kyb_bn256_scalar_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *coeffs, uint8_t *out);
int kyb_bn256_scalar_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_coeffs, void *d_out, void *stream);
int kyb_bn254_scalar_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *coeffs, uint8_t *out);
int kyb_bn254_scalar_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_coeffs, void *d_out, void *stream);
/* pairing/bn254: the same eight entry points */
int kyb_bn254_g1_msm(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t out[64], uint8_t *status, uint32_t flags);
int kyb_bn254_g2_msm(size_t n, const uint8_t *scalars, const uint8_t *points, uint8_t out[128], uint8_t *status, uint32_t flags);
int kyb_bn254_g1_msm_dev(size_t n, const void *d_scalars, const void *d_points, void *d_out, void *d_status,
                         uint32_t flags, void *stream);
int kyb_bn254_g2_msm_dev(size_t n, const void *d_scalars, const void *d_points, void *d_out, void *d_status,
                         uint32_t flags, void *stream);
int kyb_bn254_g1_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *commits, uint8_t *out,
                           uint8_t *status, uint32_t flags);
int kyb_bn254_g2_poly_eval(size_t n, const uint32_t *idx, size_t t, const uint8_t *commits, uint8_t *out,
                           uint8_t *status, uint32_t flags);
int kyb_bn254_g1_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_commits, void *d_out,
                               void *d_status, uint32_t flags, void *stream);
int kyb_bn254_g2_poly_eval_dev(size_t n, const void *d_idx, size_t t, const void *d_commits, void *d_out,
                               void *d_status, uint32_t flags, void *stream);

/* --------------------------------------------------------- sign/bdn on the pairing suites: one roster, many masks
 * <suite> is bls12381, bn256 or bn254 and <g> is g1 or g2: the KEY group (NewSchemeOnG1 keeps its keys on G2,
 * NewSchemeOnG2 on G1).  POINT is the group's MarshalBinary length: 48 / 96 on BLS12-381 (compressed), 64 / 128 on the
 * BN suites.  flags is 0 or KYB_F_TRUSTED(0), with the meaning it has in kyb_<suite>_<g>_unmarshal; any other bit is
 * KYB_E_ARG.
 *
 * kyb_<suite>_bdn_terms_<g>: what NewMask precomputes (mask.go:51-61) for a roster of m keys, in one call.
 *   coefs[j] = hashPointToR's 16 XOF bytes of key j (bdn.go:29-63): BLAKE2Xs (blake2s.NewXOF(OutputLengthUnknown, nil))
 *   over the keys' MarshalBinary bytes in roster order; read as a little-endian integer c_j they are the coefficient,
 *   whichever byte order the suite's scalars have.  terms[j] = (c_j + 1) P_j, the value of Mul(c_j, P_j) followed by
 *   Add(., P_j) (mask.go:59-60), the identity for the identity.  A key is decoded by the suite's UnmarshalBinary rules and
 *   hashed through its canonical re-encoding (bn256 reduces a coordinate at or above p; MarshalBinary writes the reduced
 *   one).  status[j] (m bytes, may be NULL) is key j's decode status in kyb_<suite>_<g>_unmarshal's codes.  If ANY key is
 *   rejected no coefficient is defined -- the hash covers the whole roster -- and every coefs and terms byte is zero;
 *   the statuses still name the rejected keys and the call returns KYB_OK.  coefs may be NULL.
 *   KYB_E_ARG before any device is touched: m = 0 or m > KYB_COSI_MAX_ROSTER, a NULL roster or terms, a flag bit other
 *   than KYB_F_TRUSTED(0).  Workspace per call: m * POINT + 64 bytes and the ladder's table slab of m lanes.
 *
 * kyb_<suite>_mask_aggregate_<g>: out[i] = the sum of the points that mask i enables, count[i] = their number:
 * AggregatePublicKeys over precomputed terms (bdn.go:166-181), where the reference makes up to m sequential Point.Add
 * calls per mask.  kyb_ed25519_mask_aggregate's scheme on a generic group: the m points are decoded once per call and
 * cut into groups of 4 or 8 with a table of every subset's sum (complete additions: equal points, opposite points and
 * the identity are points like any other); a lane adds one entry per group and a mask with more than half of its bits
 * set goes through its complement and T_all - acc.  When n alone does not fill the device a mask's groups are cut into
 * S slices, a lane per (mask, slice), and a fold pass sums the S partial sums (kyb_bdn_plan).
 *   The mask, count, stride and stray-bit rules are kyb_ed25519_mask_aggregate's: let L = (m + 7) >> 3; element i's mask
 *   is the L bytes at masks + i * mask_stride, read byte by byte, mask_stride >= L, nothing beyond the last element's L
 *   bytes is read; bit j & 7 of byte j >> 3 enables point j; bits at or above m are ignored in out and count alike.
 *   The empty mask gives the identity as kyb_<suite>_<g>_add writes it.  count (n words) and status (n bytes) may be
 *   NULL.  If a point is rejected, every status[i] is the first rejected point's status and every out[i] is zero bytes;
 *   count is the mask's own and is written anyway.
 *   KYB_E_ARG before any device is touched: m = 0 or m > KYB_COSI_MAX_ROSTER, mask_stride < L, a NULL points, masks or
 *   out with n > 0, a flag bit other than KYB_F_TRUSTED(0).  n = 0 is KYB_OK and touches nothing.
 *   Workspace per call, with E = the three Jacobian coordinates of a point as the device holds them (144 / 288 bytes on
 *   BLS12-381, 96 / 192 on the BN suites), g the table width and S the slices:
 *   (m + ((m + g - 1) / g << g) + 65 + min(n, 65536) * S) * E + m + 272 bytes; 75 MB of tables for 8192 BLS12-381 G2
 *   points at g = 8.  Addresses follow the masks, which are public.
 *
 * Both run on the current device and do not consult the device set.  _dev: device pointers, enqueued on `stream`;
 * roster, coefs, terms, points and out 16-byte aligned, count 4-byte, masks of any alignment.
 *
 * kyb_bdn_plan: plan[0] = the table width (4 or 8, kyb_ed25519_cosi_group_width's count of additions), plan[1] = the
 * slices S = min(groups, ceil(65536 / n)) a call of n masks over m points uses; touches no device.  KYB_E_ARG for n = 0,
 * m = 0, m > KYB_COSI_MAX_ROSTER or a NULL plan.
 * kyb_bdn_debug_set_slices: a measurement hook, not for production use.  slices > 0 makes every later mask_aggregate
 * call of this process use min(slices, groups) slices instead of the plan's, cut so that a piece holds at most 131 072
 * partial sums; kyb_bdn_plan keeps reporting the plan's own S.  0 restores the plan.  Touches no device. */
int kyb_bls12381_bdn_terms_g1(size_t m, const uint8_t *roster /* m x POINT */, uint8_t *coefs /* m x 16 */,
        uint8_t *terms /* m x POINT */, uint8_t *status /* m */, uint32_t flags);
int kyb_bls12381_bdn_terms_g1_dev(size_t m, const void *d_roster, void *d_coefs, void *d_terms, void *d_status,
        uint32_t flags, void *stream);
int kyb_bls12381_mask_aggregate_g1(size_t n, size_t m, const uint8_t *points /* m x POINT */, const uint8_t *masks,
        size_t mask_stride, uint8_t *out /* n x POINT */, uint32_t *count, uint8_t *status, uint32_t flags);
int kyb_bls12381_mask_aggregate_g1_dev(size_t n, size_t m, const void *d_points, const void *d_masks, size_t mask_stride,
        void *d_out, void *d_count, void *d_status, uint32_t flags, void *stream);
int kyb_bls12381_bdn_terms_g2(size_t m, const uint8_t *roster /* m x POINT */, uint8_t *coefs /* m x 16 */,
        uint8_t *terms /* m x POINT */, uint8_t *status /* m */, uint32_t flags);
int kyb_bls12381_bdn_terms_g2_dev(size_t m, const void *d_roster, void *d_coefs, void *d_terms, void *d_status,
        uint32_t flags, void *stream);
int kyb_bls12381_mask_aggregate_g2(size_t n, size_t m, const uint8_t *points /* m x POINT */, const uint8_t *masks,
        size_t mask_stride, uint8_t *out /* n x POINT */, uint32_t *count, uint8_t *status, uint32_t flags);
int kyb_bls12381_mask_aggregate_g2_dev(size_t n, size_t m, const void *d_points, const void *d_masks, size_t mask_stride,
        void *d_out, void *d_count, void *d_status, uint32_t flags, void *stream);
int kyb_bn256_bdn_terms_g1(size_t m, const uint8_t *roster /* m x POINT */, uint8_t *coefs /* m x 16 */,
        uint8_t *terms /* m x POINT */, uint8_t *status /* m */, uint32_t flags);
int kyb_bn256_bdn_terms_g1_dev(size_t m, const void *d_roster, void *d_coefs, void *d_terms, void *d_status,
        uint32_t flags, void *stream);
int kyb_bn256_mask_aggregate_g1(size_t n, size_t m, const uint8_t *points /* m x POINT */, const uint8_t *masks,
        size_t mask_stride, uint8_t *out /* n x POINT */, uint32_t *count, uint8_t *status, uint32_t flags);
int kyb_bn256_mask_aggregate_g1_dev(size_t n, size_t m, const void *d_points, const void *d_masks, size_t mask_stride,
        void *d_out, void *d_count, void *d_status, uint32_t flags, void *stream);
int kyb_bn256_bdn_terms_g2(size_t m, const uint8_t *roster /* m x POINT */, uint8_t *coefs /* m x 16 */,
        uint8_t *terms /* m x POINT */, uint8_t *status /* m */, uint32_t flags);
int kyb_bn256_bdn_terms_g2_dev(size_t m, const void *d_roster, void *d_coefs, void *d_terms, void *d_status,
        uint32_t flags, void *stream);
int kyb_bn256_mask_aggregate_g2(size_t n, size_t m, const uint8_t *points /* m x POINT */, const uint8_t *masks,
        size_t mask_stride, uint8_t *out /* n x POINT */, uint32_t *count, uint8_t *status, uint32_t flags);
int kyb_bn256_mask_aggregate_g2_dev(size_t n, size_t m, const void *d_points, const void *d_masks, size_t mask_stride,
        void *d_out, void *d_count, void *d_status, uint32_t flags, void *stream);
int kyb_bn254_bdn_terms_g1(size_t m, const uint8_t *roster /* m x POINT */, uint8_t *coefs /* m x 16 */,
        uint8_t *terms /* m x POINT */, uint8_t *status /* m */, uint32_t flags);
int kyb_bn254_bdn_terms_g1_dev(size_t m, const void *d_roster, void *d_coefs, void *d_terms, void *d_status,
        uint32_t flags, void *stream);
int kyb_bn254_mask_aggregate_g1(size_t n, size_t m, const uint8_t *points /* m x POINT */, const uint8_t *masks,
        size_t mask_stride, uint8_t *out /* n x POINT */, uint32_t *count, uint8_t *status, uint32_t flags);
int kyb_bn254_mask_aggregate_g1_dev(size_t n, size_t m, const void *d_points, const void *d_masks, size_t mask_stride,
        void *d_out, void *d_count, void *d_status, uint32_t flags, void *stream);
int kyb_bn254_bdn_terms_g2(size_t m, const uint8_t *roster /* m x POINT */, uint8_t *coefs /* m x 16 */,
        uint8_t *terms /* m x POINT */, uint8_t *status /* m */, uint32_t flags);
int kyb_bn254_bdn_terms_g2_dev(size_t m, const void *d_roster, void *d_coefs, void *d_terms, void *d_status,
        uint32_t flags, void *stream);
int kyb_bn254_mask_aggregate_g2(size_t n, size_t m, const uint8_t *points /* m x POINT */, const uint8_t *masks,
        size_t mask_stride, uint8_t *out /* n x POINT */, uint32_t *count, uint8_t *status, uint32_t flags);
int kyb_bn254_mask_aggregate_g2_dev(size_t n, size_t m, const void *d_points, const void *d_masks, size_t mask_stride,
        void *d_out, void *d_count, void *d_status, uint32_t flags, void *stream);
int kyb_bdn_plan(size_t n, size_t m, int plan[2] /* width, slices */);
int kyb_bdn_debug_set_slices(size_t slices);

#ifdef __cplusplus
}
#endif
#endif
