// sign/bdn on BLS12-381: NewMask's coefficients and terms, and the masked sums of AggregatePublicKeys, for keys on G1 or
// on G2 -- bdn_launch.cuh's kernels over bls::G1 / bls::G2 and their C-ABI entry points.  A unit of its own, so that the
// suite's other units keep their kernels and their register allocation.  Both calls run on the current device.
#include "bls12381.cuh"
#include "pairing_abi.cuh"
#include "bdn_launch.cuh"

KYB_EXPORT_BDN_ABI(bls12381, kyb::bls::Suite)
