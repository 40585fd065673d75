"""One rank of a sharded proof whose instance was ingested on the device (tests/test_gpu_snark_from_device.py starts several of these as child
processes): shard_worker.py's `prove` and `snark` with Instance.from_zkif(..., mode="device") in place of Instance.new.  The last line printed is
the instance's host_lists_info() as JSON.
usage: shard_zkif_worker.py prove  <segment> <rank> <world> <out.bin> <zkif prefix>
       shard_zkif_worker.py snark  <segment> <rank> <world> <out.bin> <zkif prefix>   (SNARK mode: commitment bytes + proof bytes)
       shard_zkif_worker.py encode <out.bin> <zkif prefix>                            (no ranks: the commitment of the device-ingested instance)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import otti_amd as oa  # noqa: E402
from shard_worker import SEED, LABEL  # noqa: E402


def ingest(prefix):
    inst, a = oa.Instance.from_zkif(prefix + ".zkif", prefix + ".inp.zkif", prefix + ".wit.zkif", mode="device")
    assert inst.ingest_info()["on_device"] and not inst.host_lists_info()["materialised"]
    return inst, a


def prove(seg, rank, world, out, prefix):
    inst, a = ingest(prefix)
    gens = oa.NIZKGens.new(a["num_cons"], a["num_vars"], a["num_inputs"])
    wit = oa.Witness(inst, oa.VarsAssignment.new(a["vars"]), oa.InputsAssignment.new(a["inputs"]))
    oa.shard_init(seg, rank, world)
    pf = oa.NIZK.prove_sharded(inst, wit, gens, LABEL, SEED)
    oa.shard_finalize()
    open(out, "wb").write(pf.bytes)
    return inst


def snark(seg, rank, world, out, prefix):
    inst, a = ingest(prefix)
    gens = oa.SNARKGens.new(a["num_cons"], a["num_vars"], a["num_inputs"], max(a["nA"], a["nB"], a["nC"]))
    comm = oa.ComputationCommitment.encode(inst, gens)          # every rank encodes, from the lists in HBM
    wit = oa.Witness(inst, oa.VarsAssignment.new(a["vars"]), oa.InputsAssignment.new(a["inputs"]))
    oa.shard_init(seg, rank, world)
    pf = oa.SNARK.prove_sharded(inst, comm, wit, gens, LABEL, SEED)
    oa.shard_finalize()
    open(out, "wb").write(len(comm.bytes).to_bytes(8, "little") + comm.bytes + pf.bytes)
    return inst


def encode(out, prefix):
    inst, a = ingest(prefix)
    gens = oa.SNARKGens.new(a["num_cons"], a["num_vars"], a["num_inputs"], max(a["nA"], a["nB"], a["nC"]))
    open(out, "wb").write(oa.ComputationCommitment.encode(inst, gens).bytes)
    return inst


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "encode":
        inst = encode(sys.argv[2], sys.argv[3])
    else:
        inst = (snark if mode == "snark" else prove)(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6])
    print(json.dumps(inst.host_lists_info()))
