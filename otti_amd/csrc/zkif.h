// The frame both zkInterface loaders share (zkif.cpp): headers, witness message, id map, the walk over the circuit file's messages, and — behind
// the loader's own pass over the constraints — the assignment.  The host loader (zkif_load_impl) parses the constraints into otti_entry lists
// with host threads; the device loader (k_ingest.hip) ships the ConstraintSystem messages to HBM as they are in the file and parses them there.
#pragma once
#include "spartan.h"
#include "zkif_walk.h"
#include <functional>
#include <vector>

namespace otti {

// what a constraint pass is given: the circuit file's mapping, its ConstraintSystem messages in file order (ZwMsg::base points into the mapping;
// the offset vector of each is known to lie within its message) and the id map
struct ZkifCircuit {
    const uint8_t *file = nullptr; size_t file_bytes = 0;
    std::vector<ZwMsg> msgs; uint64_t rows = 0;
    const uint32_t *col_of = nullptr; size_t n_ids = 0;       // IdMap::col_of: 0xffffffff = undeclared
    size_t num_vars = 0, num_inputs = 0;
};
typedef std::function<void(const char *)> ZkifLap;           // a lap of the loader's OTTI_TRACE timing
// pass(circuit, out, lap): out's dimensions are filled after it; the host pass fills A, B, C and their counts, a device pass the counts alone
typedef std::function<void(const ZkifCircuit &, otti_r1cs *, const ZkifLap &)> ZkifConstraintPass;
otti_r1cs *zkif_load_with(const char *circuit_path, const char *inputs_path, const char *witness_path, const ZkifConstraintPass &pass);

}  // namespace otti
