"""ctypes binding of libkyberhip.so (the C ABI in include/kyber_hip.h).

Fails loudly when the library is absent or a symbol is missing: there is no
CPU fallback in the product path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KYBER_HIP_LIB") or os.path.join(_HERE, "lib", "libkyberhip.so")  # override: A/B builds

KYB_F_VARTIME = 1
KYB_F_UNIFORM = 8  # Ed25519: scalar-independent addresses and control flow (include/kyber_hip.h)
KYB_F_DLEQ_FS = 16  # kyb_ed25519_dleq_verify: C[i] must equal the challenge derived on the device
ST_OK, ST_BAD_POINT, ST_NOT_IN_SUBGROUP = 0, 1, 2
ST_IBE_CHECK, ST_IBE_H3 = 3, 4  # encrypt/ibe: rP != U; h3's rejection sampling exhausted
E_EXHAUSTED = -5  # kyb_ed25519_xof_pick: the window of candidate draws held fewer than n scalars
ST_DLEQ_CHALLENGE, ST_PICK_EXHAUSTED = 7, 8  # proof/dleq: challenge mismatch; Scalar.Pick's rejection loop exhausted
ST_ECIES_SHORT, ST_ECIES_AUTH = 9, 10  # encrypt/ecies Decrypt: shorter than R and a tag; the tag does not match
ST_ANON_SHORT, ST_ANON_INVALID, ST_ANON_MAC = 11, 12, 13  # sign/anon Decrypt: too short; invalid ciphertext; failed MAC check
# sign/dss ProcessPartialSig: index outside the roster; the signature's equation; the session id; V B against the commitments
ST_DSS_INDEX, ST_DSS_SIG, ST_DSS_SESSION, ST_DSS_PARTIAL = 14, 15, 16, 17
ANON_MAX_RING = 4096  # KYB_ANON_MAX_RING


class KyberHipError(RuntimeError):
    pass


_vp, _sz, _u32, _u64, _int = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int

# Rows with a device twin: NAME_dev takes the same arguments plus the stream (a void *).
_n4 = [_sz, _vp, _vp, _vp, _vp]  # n and four buffers
_n6 = [_sz, _vp, _vp, _vp, _vp, _vp, _vp]
_hash = [_sz, _vp, _sz, _vp, _sz, _vp, _vp]  # n, msgs, msg_len, dst, dst_len, out, status
_verify = [_sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _u32]
_ibe_enc = [_sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _u32]
_ibe_dec = [_sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _u32]
_BOTH = {
    "kyb_ed25519_mul_base": [_sz, _vp, _vp, _u32],
    "kyb_ed25519_mul": _n4 + [_u32],
    "kyb_ed25519_verify": _n6 + [_u32],
    "kyb_ed25519_mul2": _n6 + [_u32],
    "kyb_ed25519_dleq_challenge": _n6,
    "kyb_ed25519_dleq_verify": [_sz, _vp, _sz, _vp, _sz] + [_vp] * 9 + [_u32],
    "kyb_ed25519_xof_pick": [_sz, _vp, _u64, _vp, _vp],
    "kyb_ed25519_theta_check": [_sz] + [_vp] * 9 + [_u32],
    "kyb_ed25519_lincomb": [_sz, _sz, _sz, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32],
    "kyb_ed25519_fs_challenge": [_sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp],
    "kyb_ed25519_mask_aggregate": [_sz, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _u32],
    "kyb_ed25519_cosi_verify": [_sz, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _u32],
    "kyb_ed25519_ecies_seal": [_sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp],
    "kyb_ed25519_ecies_open": [_sz, _vp, _sz, _vp, _vp, _vp, _vp],
    "kyb_ed25519_deal_check": [_sz, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp],
    "kyb_ed25519_schnorr_sign": [_sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp],
    "kyb_ed25519_vss_seal": [_sz, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "kyb_ed25519_vss_open": [_sz, _vp, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp],
    "kyb_ed25519_deal_check2": [_sz, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp],
    "kyb_ed25519_dss_check": [_sz, _sz, _vp, _sz, _vp, _sz, _sz] + [_vp] * 11,
    "kyb_ed25519_dss_partial": [_sz, _vp, _u32, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "kyb_ed25519_eddsa_expand": [_sz, _vp, _vp, _vp, _vp],
    "kyb_ed25519_eddsa_sign": [_sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp],
    "kyb_ed25519_anon_seal": [_sz, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "kyb_ed25519_anon_open": [_sz, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp],
    "kyb_ed25519_ring_chain": [_sz, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _u32],
    "kyb_ed25519_ring_challenge": [_sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "kyb_ed25519_add": _n4,
    "kyb_ed25519_hash": _hash[:-1],  # no status
    "kyb_ed25519_msm": _n4,
    "kyb_ed25519_unmarshal": [_sz, _vp, _vp, _vp],
    "kyb_ed25519_poly_eval": [_sz, _vp, _sz, _vp, _vp, _vp],
    "kyb_ed25519_scalar_poly_eval": [_sz, _vp, _sz, _vp, _vp],
    "kyb_bls12381_hash_g1": _hash,
    "kyb_bls12381_hash_g2": _hash,
    "kyb_bls12381_verify_g1": _verify,
    "kyb_bls12381_verify_g2": _verify,
    "kyb_bls12381_verify_g1_same_key": _verify,
    "kyb_bls12381_verify_g1_same_msg": _verify,
    "kyb_bls12381_ibe_encrypt_g1": _ibe_enc,
    "kyb_bls12381_ibe_encrypt_g2": _ibe_enc,
    "kyb_bls12381_ibe_decrypt_g1": _ibe_dec,
    "kyb_bls12381_ibe_decrypt_g2": _ibe_dec,
    "kyb_bn256_hash_g1": [_sz, _vp, _sz, _vp, _vp],  # the reference's own hash: no DST
    "kyb_bn256_hash_g1_svdw": _hash,
    "kyb_bn254_hash_g1": _hash,
}
# Host only.
_HOST_ONLY = {
    "kyb_version": [],
    "kyb_last_error": [],
    "kyb_device_count": [],
    "kyb_init": [],
    "kyb_shutdown": [],
    "kyb_stream_release": [_vp],
    "kyb_init_devices": [_int],
    "kyb_set_devices": [_vp, _int],
    "kyb_get_devices": [_vp, _int],
    "kyb_set_shard_threshold": [_sz],
    "kyb_shard_range": [_sz, _int, _int, _vp, _vp],
    "kyb_ed25519_mul_same_base": _n4 + [_u32],
    "kyb_ed25519_cosi_group_width": [_sz, _sz],
    "kyb_bdn_plan": [_sz, _sz, _vp],
    "kyb_bdn_debug_set_slices": [_sz],
    "kyb_ed25519_msm_flags": _n4 + [_u32],
    "kyb_ed25519_debug_base_table": [_vp],
    "kyb_ed25519_comb_info": [_vp],
    "kyb_ed25519_debug_comb_table": [_int, _int, _int, _vp],
    "kyb_bls12381_debug_vkey_stats": [_vp, _vp],
}
# What every pairing suite has, kyb_<suite>_<suffix>; "g?" stands for g1 and g2.  Each has a device twin as above.
_SUITES = ("bls12381", "bn256", "bn254")
_PER_SUITE = {
    "g?_msm": _n4 + [_u32],
    "g?_mul": _n4 + [_u32],
    "g?_add": _n4,
    "g?_unmarshal": [_sz, _vp, _vp, _vp, _u32],
    "g?_poly_eval": [_sz, _vp, _sz, _vp, _vp, _vp, _u32],
    "scalar_poly_eval": [_sz, _vp, _sz, _vp, _vp],
    "pair": _n4 + [_u32],
    "pair_check": _n6 + [_u32],
    "gt_mul": _n4,
    "bdn_terms_g?": [_sz, _vp, _vp, _vp, _vp, _u32],  # m, roster, coefs, terms, status, flags
    "mask_aggregate_g?": [_sz, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _u32],  # as kyb_ed25519_mask_aggregate
}


def _signatures() -> dict:
    """name -> argtypes; restype is int unless listed in _RESTYPES"""
    both = dict(_BOTH)
    sigs = dict(_HOST_ONLY)
    for suite in _SUITES:
        for suffix, args in _PER_SUITE.items():
            for g in ("g1", "g2") if "g?" in suffix else ("",):
                both[f"kyb_{suite}_{suffix.replace('g?', g)}"] = args
        for g in ("g1", "g2"):  # one base for the batch has an entry point of its own on the host, a stride on the device
            sigs[f"kyb_{suite}_{g}_mul_same_base"] = _n4 + [_u32]
    for name, args in both.items():
        sigs[name] = list(args)
        sigs[name + "_dev"] = args + [_vp]
    for suite in _SUITES:
        for g in ("g1", "g2"):  # n, scalars, points, point stride, out, status, flags, stream
            sigs[f"kyb_{suite}_{g}_mul_dev"] = [_sz, _vp, _vp, _sz, _vp, _vp, _u32, _vp]
    return sigs


SIGNATURES = _signatures()
_RESTYPES = {"kyb_last_error": C.c_char_p, "kyb_shard_range": None}

_lib = None


def load() -> C.CDLL:
    """Load (once) and return the library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KyberHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # PyTorch-ROCm ships its own HIP runtime.  If libkyberhip.so pulled in the system one first, a later
    # `import torch` would find a HIP runtime it did not initialise and report no usable device
    # (torch.cuda.is_available() == False): let torch's copy load first whenever torch is installed.
    try:
        import torch  # noqa: F401
    except ImportError:  # pure host-buffer use without torch
        pass
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise KyberHipError(f"libkyberhip.so lacks symbol {name}") from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, C.c_int)
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().kyb_last_error()
        raise KyberHipError(f"{what} failed rc={rc}: {msg.decode() if msg else ''}")
