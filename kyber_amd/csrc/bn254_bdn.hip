// sign/bdn on bn254: NewMask's coefficients and terms, and the masked sums of AggregatePublicKeys, for keys on G1 or on
// G2 -- bdn_launch.cuh's kernels over bn4::G1 / bn4::G2 and their C-ABI entry points.  A unit of its own, so that the
// suite's other units keep their kernels and their register allocation.  Both calls run on the current device.
#ifndef KYB_TU_WAVES
#define KYB_TU_WAVES 2
#endif
#include "bn254.cuh"
#include "pairing_abi.cuh"
#include "bdn_launch.cuh"

KYB_EXPORT_BDN_ABI(bn254, kyb::bn4::Suite)
