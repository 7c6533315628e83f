// zl_host_api.h -- the two handles behind the host-mirror C hooks (include/zl_backend.h), for the units that implement those hooks: zl_host.hip (circuits, keys,
// proving, wire formats) and zl_verify.hip (verification).  Internal; nothing else belongs here.
#pragma once
#include "zl_host.h"

struct zl_circuit {
    zl_curve_t curve;
    openzl::R1CS<BLS12_381_Fr>* bls = nullptr;
    openzl::R1CS<BN254_Fr>* bn = nullptr;
    openzl::R1csExport<BLS12_381_Fr> ex_bls;
    openzl::R1csExport<BN254_Fr> ex_bn;
};
struct zl_g16_keys {
    zl_curve_t curve;
    openzl::Groth16<openzl::Bls12_381>::ProvingContext pc_bls;
    openzl::Groth16<openzl::Bn254>::ProvingContext pc_bn;
    std::vector<uint64_t> gamma_abc;  // exponents, canonical
    openzl::Groth16<openzl::Bls12_381>::VerifyingContext vk_bls;
    openzl::Groth16<openzl::Bn254>::VerifyingContext vk_bn;
};
