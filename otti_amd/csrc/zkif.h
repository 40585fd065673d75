// The frame both zkInterface loaders share (zkif.cpp): headers, witness message, id map, the walk over the circuit file's messages, and — behind
// the loader's own pass over the constraints — the assignment.  The host loader (zkif_load_impl) parses the constraints into otti_entry lists
// with host threads; the device loader (k_ingest.hip) ships the ConstraintSystem messages to HBM as they are in the file and parses them there.
#pragma once
#include "spartan.h"
#include "zkif_walk.h"
#include "zkif_wit_walk.h"
#include <functional>
#include <string>
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

// ---- the assignment alone, from the .inp.zkif and the .wit.zkif without a circuit file (otti_witness_from_zkif).  The id map comes from these two
// files: the instance ids and free_variable_id of the inputs header, the witness ids.  want_dims (optional): {num_vars, num_inputs} the caller's
// instance has; other dimensions are OTTI_ERR_BAD_ARG, said behind the frame's own checks of headers, id map and count and before any value is
// looked at.  Every other check, its order and its code are zkif_load's for the same two files beside a clean circuit.
// The host loader: the frame's pieces with the circuit's left out; only num_vars, num_inputs, vars32, nvars, inputs32, ninputs are filled.
otti_r1cs *zkif_load_assignment(const char *inputs_path, const char *witness_path, const size_t want_dims[2]);
// The device loader's frame: the inputs file parsed as ever; the Witness messages of the witness file located and checked (zkif_wit_walk.h WwMsg:
// base points into the mapping), their values never copied; every check that needs no value made here.  The host's own first defect, when the
// values could still hold an earlier one, is handed on as `seed`: the pass starts its smallest key from it.
struct ZkifWitness {
    std::vector<WwMsg> msgs; uint64_t total = 0;              // Witness messages in file order; assigned variables over all of them
    bool have_witness = false;                                // a Witness message exists (none: no variable is assigned, as zkif_load leaves nvars = 0)
    std::vector<uint64_t> inst_sorted;                        // the instance ids, ascending
    size_t num_vars = 0, num_inputs = 0, witness_bytes = 0;
    std::vector<uint8_t> inputs32; std::vector<Fr> inputs;    // the public inputs: canonical bytes, and Montgomery form unless the seed says they are not canonical
    uint64_t seed = kZwNoError; int seed_code = OTTI_OK; std::string seed_what;
};
typedef std::function<void(const ZkifWitness &)> ZkifWitnessPass;
void zkif_witness_with(const char *inputs_path, const char *witness_path, const size_t want_dims[2], const ZkifWitnessPass &pass);
[[noreturn]] void zkif_witness_refuse(const ZkifWitness &zw, uint64_t key);   // the Error a pass's smallest key stands for

// ---- what the two device loaders share (k_ingest.hip): message bodies laid out 16-byte aligned in one image, staged through the process's pinned slabs
struct IngestMsg { unsigned long long off, size, vec_start, count, first_row; };   // ZwMsg with the body's place in the staged image
struct DevCtx;
void ingest_stage_image(DevCtx &c, uint8_t *d_image, size_t image_bytes, const std::vector<ZwMsg> &msgs, const std::vector<IngestMsg> &lay);

}  // namespace otti
