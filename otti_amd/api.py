"""ctypes binding of libottispartan.so — same names, argument meaning and error behaviour as upstream libspartan's
`src/lib.rs` for the NIZK path [RECALL], which is what `spzk verify --nizk` [REF /root/reference/run.py:58,100] and
rust-circ `--action spartan` [REF /root/reference/run.py:147] call."""
import contextlib
import ctypes
import os
import sys
import numpy as np

L_ORDER = 2 ** 252 + 27742317777372353535851937790883648493
_R = (1 << 256) % L_ORDER
_RINV = pow(_R, -1, L_ORDER)

ENTRY_DTYPE = np.dtype([("row", "<u8"), ("col", "<u8"), ("val", "u1", (32,))])   # otti_entry

_HERE = os.path.dirname(os.path.abspath(__file__))
lib_path = os.path.join(_HERE, "libottispartan.so")


class SpartanError(Exception):
    def __init__(self, code, msg=""):
        super().__init__(f"{type(self).__name__}({code}): {msg}")
        self.code = code


class R1CSError(SpartanError):
    """upstream R1CSError: InvalidNumberOfInputs(-3) InvalidNumberOfVars(-4) InvalidScalar(-5) InvalidIndex(-6)"""


class ProofVerifyError(SpartanError):
    """upstream ProofVerifyError: InternalError(-10) DecompressionError(-11); -12 = malformed proof bytes"""


class NoDeviceError(SpartanError):
    """no gfx950 device or HIP failure — the proving path has no CPU fallback"""


def _load():
    if not os.path.exists(lib_path):
        raise ImportError(
            f"{lib_path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C otti_amd/csrc). otti_amd has no pure-Python or CPU fallback.")
    return ctypes.CDLL(lib_path)


lib = _load()
_sz, _u64, _i32, _vp = ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p
_u8p = ctypes.POINTER(ctypes.c_uint8)


class _R1CS(ctypes.Structure):
    _fields_ = [("num_cons", _u64), ("num_vars", _u64), ("num_inputs", _u64),
                ("A", _vp), ("B", _vp), ("C", _vp), ("nA", _sz), ("nB", _sz), ("nC", _sz),
                ("vars32", _vp), ("nvars", _sz), ("inputs32", _vp), ("ninputs", _sz)]


class _DeviceInfo(ctypes.Structure):
    _fields_ = [("rows", _u64), ("entries", _u64 * 3), ("n_heavy", _u64), ("n_seg", _u64), ("use_small", _i32), ("quad", _i32)]


def _sig(name, res, *args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


_sig("otti_last_error", _sz, ctypes.c_char_p, _sz)
_sig("otti_buf_free", None, _vp)
_sig("otti_device_count", _i32)
_sig("otti_host_selftest", _i32, ctypes.c_uint32)
_sig("otti_host_microbench", _i32, ctypes.POINTER(ctypes.c_double))
_sig("otti_host_point_from_uniform", _i32, _vp, _vp)
_sig("otti_host_point_sum", _i32, _vp, _sz, _i32, ctypes.c_uint32, _vp)
_sig("otti_host_point_sum_bench", _i32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double))
_sig("otti_host_tail_bench", _i32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double))
_sig("otti_instance_new", _i32, _u64, _u64, _u64, _vp, _sz, _vp, _sz, _vp, _sz, ctypes.POINTER(_vp))
_sig("otti_instance_free", None, _vp)
_sig("otti_instance_dims", _i32, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64))
_sig("otti_instance_is_sat", _i32, _vp, _vp, _sz, _vp, _sz, ctypes.POINTER(_i32))
_sig("otti_gens_new", _i32, _u64, _u64, _u64, ctypes.POINTER(_vp))
_sig("otti_gens_free", None, _vp)
_sig("otti_gens_points", _i32, _vp, _vp, _sz)
_sig("otti_gens_table_info", _i32, _vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_u64))
_sig("otti_nizk_prove", _i32, _vp, _vp, _sz, _vp, _sz, _vp, ctypes.c_char_p, _sz, _vp, ctypes.c_uint32,
     ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_double))
_sig("otti_witness_upload", _i32, _vp, _vp, _sz, _vp, _sz, ctypes.POINTER(_vp))
_sig("otti_witness_free", None, _vp)
_sig("otti_witness_from_device", _i32, _vp, _vp, _sz, _i32, _sz, _vp, _sz, _vp, ctypes.POINTER(_vp))
_sig("otti_witness_upload_ints", _i32, _vp, _vp, _sz, _i32, _vp, _sz, ctypes.POINTER(_vp))
_sig("otti_witness_update", _i32, _vp, _vp, _sz, _vp, _sz, _i32, _sz, _i32, _vp)
_sig("otti_witness_scatter", _i32, _vp, _vp, _vp, _vp, _sz, _i32, _sz, _i32, _vp)
_sig("otti_witness_scatter_info", _i32, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64))
_sig("otti_witness_assign", _i32, _vp, _vp, _sz, _vp, _sz, _i32, _sz, _i32, _vp, ctypes.POINTER(_u64))
_sig("otti_witness_diff", _i32, _vp, _vp, _sz, _vp, _sz, _i32, _sz, _i32, _vp, ctypes.POINTER(_u64), _vp, _sz)
_sig("otti_witness_assign_info", _i32, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64))
_sig("otti_witness_set_inputs", _i32, _vp, _vp, _vp, _sz)
_sig("otti_witness_info", _i32, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_double))
_sig("otti_witness_keep_rows", _i32, _vp, _vp, _vp)
_sig("otti_witness_keep_rows_snark", _i32, _vp, _vp, _vp)
_sig("otti_witness_drop_rows", _i32, _vp)
_sig("otti_witness_rows_info", _i32, _vp, ctypes.POINTER(_i32), ctypes.POINTER(_sz), ctypes.POINTER(_sz), ctypes.POINTER(_u64))
_sig("otti_witness_keep_products", _i32, _vp, _vp)
_sig("otti_witness_drop_products", _i32, _vp)
_sig("otti_witness_products_info", _i32, _vp, ctypes.POINTER(_i32), ctypes.POINTER(_sz), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
     ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64))
_sig("otti_witness_check_sat", _i32, _vp, _vp, ctypes.POINTER(_u64), _vp, _sz, _vp, ctypes.POINTER(ctypes.c_float))
_sig("otti_nizk_prove_resident", _i32, _vp, _vp, _vp, ctypes.c_char_p, _sz, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz),
     ctypes.POINTER(ctypes.c_double))
_sig("otti_shard_init", _i32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32)
_sig("otti_shard_finalize", _i32)
_sig("otti_shard_info", _i32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32))
_sig("otti_shard_allgather", _i32, _vp, _sz, _vp)
_sig("otti_shard_allreduce", _i32, _vp, _sz)
_sig("otti_nizk_prove_sharded", _i32, _vp, _vp, _vp, ctypes.c_char_p, _sz, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz),
     ctypes.POINTER(ctypes.c_double))
_sig("otti_nizk_verify", _i32, _vp, _vp, _sz, _vp, ctypes.c_char_p, _sz, _vp, _sz)
_sig("otti_nizk_verify_many", _i32, _vp, _vp, ctypes.c_char_p, _sz, _sz, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(_vp), ctypes.POINTER(_sz),
     ctypes.c_uint32, ctypes.POINTER(_i32), ctypes.POINTER(_sz))
class _VerifyBatchInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("live", "equations", "points", "gen_slots", "on_device", "accepted_first_pass", "localise_passes", "singles_rerun",
                                               "workers", "routed_to_many")] + [("sum_ms", ctypes.c_double)]
_sig("otti_nizk_verify_batch", _i32, _vp, _vp, ctypes.c_char_p, _sz, _sz, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(_vp), ctypes.POINTER(_sz),
     ctypes.c_uint32, _vp, ctypes.POINTER(_i32), ctypes.POINTER(_sz), ctypes.POINTER(_VerifyBatchInfo))
class _ProveManyInfo(ctypes.Structure):
    _fields_ = [("chunks", ctypes.c_uint32), ("product_tiles", ctypes.c_uint32), ("row_jobs", ctypes.c_uint32), ("workers", ctypes.c_uint32),
                ("rows_from_front", ctypes.c_uint32), ("products_from_front", ctypes.c_uint32), ("front_failed", ctypes.c_uint32),
                ("row_kernel", _i32 * 4), ("front_ms", ctypes.c_double * 3)]

    def as_dict(self):
        names = ("bulk", "bulk_sparse", "small")
        d = {k: int(getattr(self, k)) for k in ("chunks", "product_tiles", "row_jobs", "workers", "rows_from_front", "products_from_front", "front_failed")}
        d["row_kernel"] = [names[k] for k in self.row_kernel if k >= 0]
        d["front_ms"] = dict(zip(("staging", "row_sums", "products"), self.front_ms))
        return d


_sig("otti_nizk_prove_many", _i32, _vp, ctypes.POINTER(_vp), _sz, _vp, ctypes.c_char_p, _sz, ctypes.POINTER(_vp), ctypes.c_uint32,
     ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(_i32), ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_ProveManyInfo))
_sig("otti_prepare_device", _i32, _vp, _vp)
_sig("otti_snark_gens_new", _i32, _u64, _u64, _u64, _u64, ctypes.POINTER(_vp))
_sig("otti_snark_gens_free", None, _vp)
_sig("otti_snark_encode", _i32, _vp, _vp, ctypes.POINTER(_vp))
_sig("otti_comp_comm_bytes", _i32, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz))
_sig("otti_comp_comm_from_bytes", _i32, _vp, _sz, ctypes.POINTER(_vp))
_sig("otti_comp_comm_free", None, _vp)
_sig("otti_comp_comm_attach", _i32, _vp, _vp, _vp, ctypes.c_uint32)
_sig("otti_comp_comm_dims", _i32, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_i32))
_sig("otti_snark_gens_points", _i32, _vp, _i32, _vp, _sz, ctypes.POINTER(_sz))
_sig("otti_snark_prove", _i32, _vp, _vp, _vp, _sz, _vp, _sz, _vp, ctypes.c_char_p, _sz, _vp, ctypes.c_uint32,
     ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_double))
_sig("otti_snark_prove_resident", _i32, _vp, _vp, _vp, _vp, ctypes.c_char_p, _sz, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_double))
_sig("otti_snark_prove_sharded", _i32, _vp, _vp, _vp, _vp, ctypes.c_char_p, _sz, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_double))
_sig("otti_snark_verify", _i32, _vp, _vp, _sz, _vp, ctypes.c_char_p, _sz, _vp, _sz)
_sig("otti_snark_verify_many", _i32, _vp, _vp, ctypes.c_char_p, _sz, _sz, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(_vp), ctypes.POINTER(_sz),
     ctypes.c_uint32, ctypes.POINTER(_i32), ctypes.POINTER(_sz))
_sig("otti_snark_verify_batch", _i32, _vp, _vp, ctypes.c_char_p, _sz, _sz, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(_vp), ctypes.POINTER(_sz),
     ctypes.c_uint32, _vp, ctypes.POINTER(_i32), ctypes.POINTER(_sz), ctypes.POINTER(_VerifyBatchInfo))
_sig("otti_zkif_load", _i32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.POINTER(_R1CS)))
_sig("otti_zkif_write", _i32, ctypes.POINTER(_R1CS), ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p)
_sig("otti_r1cs_free", None, ctypes.POINTER(_R1CS))
_sig("otti_synth_r1cs", _i32, _u64, _u64, _u64, ctypes.POINTER(ctypes.POINTER(_R1CS)))
_sig("otti_synth_r1cs_compiler_like", _i32, _u64, _u64, _u64, ctypes.POINTER(ctypes.POINTER(_R1CS)))
_sig("otti_bench_madd_peak", _i32, ctypes.POINTER(ctypes.c_double))
_sig("otti_stats_enable", _i32, _i32)
_sig("otti_stats_select", _i32, ctypes.c_char_p)
_sig("otti_armed_launches_on", _i32, ctypes.POINTER(_i32))
_sig("otti_gens_release_device", _i32, _vp)
_sig("otti_gens_adopt_table", _i32, _vp, _vp)
_sig("otti_gens_table_users", _i32, _vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_void_p))
_sig("otti_gens_build_ms", _i32, _vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double))
_sig("otti_bench_fr_mul_peak", _i32, ctypes.POINTER(ctypes.c_double))
_sig("otti_stats_read", _i32, ctypes.c_char_p, ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double))
_sig("otti_lanes_pack", None, _vp, _sz, _vp)
_sig("otti_lanes_unpack", None, _vp, _sz, _vp)
_fp = ctypes.POINTER(ctypes.c_float)
_sig("otti_k_fr_op", _i32, _i32, _vp, _vp, _vp, _sz, _fp)
_sig("otti_k_fr_from_canonical", _i32, _vp, _vp, _sz)
_sig("otti_k_addr_timestamps", _i32, _vp, _sz, _sz, _vp, _vp, _fp)
_sig("otti_k_fr_to_canonical", _i32, _vp, _vp, _sz)
_sig("otti_k_multiply_vec", _i32, _vp, _vp, _vp, _vp, _vp, _fp)
_sig("otti_k_multiply_vec_many", _i32, _vp, ctypes.POINTER(_vp), _sz, _vp, _vp, _vp, _fp)
_sig("otti_k_prove_front", _i32, _vp, _vp, ctypes.POINTER(_vp), _vp, _sz, _vp, _vp, _vp, _vp, ctypes.POINTER(_ProveManyInfo), _fp)
_sig("otti_k_eval_table_sparse", _i32, _vp, _vp, _vp, _vp, _fp)
_sig("otti_k_products_patch", _i32, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp, ctypes.POINTER(_u64), _vp, _sz, ctypes.POINTER(_u64), ctypes.POINTER(_i32), _fp)
_sig("otti_instance_device_info", _i32, _vp, _i32, ctypes.POINTER(_DeviceInfo))
_sig("otti_k_instance_evaluate", _i32, _vp, _vp, _vp, _sz, _vp, _fp)
_sig("otti_instance_from_zkif", _i32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, _i32, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.POINTER(_R1CS)))
_sig("otti_instance_entries", _i32, _vp, _i32, _vp, _sz, ctypes.POINTER(_sz))
_sig("otti_instance_ingest_info", _i32, _vp, ctypes.POINTER(_i32), ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double))
_sig("otti_instance_host_lists_info", _i32, _vp, ctypes.POINTER(_i32), ctypes.POINTER(_u64))
class _Coo(ctypes.Structure):                                  # otti_coo
    _fields_ = [("row", _vp), ("col", _vp), ("val", _vp), ("n", _sz), ("index_format", _i32), ("val_format", _i32), ("val_stride_bytes", _sz)]


IDX_U32, IDX_I32, IDX_U64, IDX_I64 = 0, 1, 2, 3                # OTTI_IDX_*
_sig("otti_instance_from_coo", _i32, _u64, _u64, _u64, ctypes.POINTER(_Coo), _i32, _vp, ctypes.POINTER(_vp))
_sig("otti_instance_device_entries", _i32, _vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_sz))
class _CooValues(ctypes.Structure):                            # otti_coo_values
    _fields_ = [("val", _vp), ("n", _sz), ("val_format", _i32), ("val_stride_bytes", _sz)]


_sig("otti_instance_set_values", _i32, _vp, ctypes.POINTER(_CooValues), _i32, _vp)
_sig("otti_instance_values_info", _i32, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_i32), ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double))
_sig("otti_k_instance_values_kernel_ms", _i32, _vp, _fp)
_sig("otti_comp_comm_revalue", _i32, _vp, _vp, _vp)
_sig("otti_k_decomm_entries", _i32, _vp, _vp, _vp, _sz, _sz, _sz, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _fp)
_sig("otti_k_shard_filter", _i32, _vp, _vp, _vp, _sz, ctypes.c_uint32, ctypes.c_uint32, _i32, _vp, _vp, _vp, ctypes.POINTER(_sz), _fp)
INGEST_MODES = {"auto": 0, "host": 1, "device": 2}             # OTTI_INGEST_*
_sig("otti_witness_from_zkif", _i32, _vp, ctypes.c_char_p, ctypes.c_char_p, _i32, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.POINTER(_R1CS)))
_sig("otti_witness_ingest_min_mb", ctypes.c_double)
_sig("otti_witness_ingest_info", _i32, _vp, ctypes.POINTER(_i32), ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double))
_sig("otti_k_eq_evals", _i32, _vp, _sz, _vp, _fp)
_sig("otti_k_fold_top", _i32, _vp, _sz, _vp, _vp, _fp)
_sig("otti_k_fold_bot", _i32, _vp, _sz, _vp, _vp, _fp)
_sig("otti_k_sc_cubic_round", _i32, _vp, _vp, _vp, _vp, _sz, _vp, _fp)
_sig("otti_k_sc_cubic_fold_round", _i32, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _fp)
_sig("otti_k_sc_quad_round", _i32, _vp, _vp, _sz, _vp, _fp)
_sig("otti_k_sc_quad_fold_round", _i32, _vp, _vp, _sz, _vp, _vp, _vp, _fp)
_sig("otti_k_armed_selftest", _i32, _vp, _vp, _sz, _vp, ctypes.c_uint32, _vp, _vp)
_sig("otti_k_sc_caps_override", _i32, _vp)
_sig("otti_k_sc_plan", _i32, _i32, _sz, _i32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_u64))
_sig("otti_k_msm_rows", _i32, _vp, _vp, _sz, _sz, _vp, _vp, _fp)
_sig("otti_k_msm_job", _i32, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _i32, _i32, _i32, _sz, _vp, _vp, _fp)
_sig("otti_k_row_sum", _i32, _vp, _sz, _vp, _vp)
_sig("otti_k_row_sum_many", _i32, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp)
_sig("otti_k_batch_sum", _i32, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp)
_sig("otti_k_gen_runs", _i32, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp)
_sig("otti_k_msm_scatter_rows", _i32, _vp, _sz, _vp, _vp, _sz, _vp, _fp)
_sig("otti_k_witness_diff", _i32, _vp, _sz, _vp, _i32, _sz, _vp, _vp, _vp, ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_uint32), _fp)
_sig("otti_k_eq_pyramid", _i32, _vp, _sz, _vp)
_sig("otti_k_sc_cubic3_round", _i32, _vp, _vp, _vp, _sz, _vp, _vp, _fp)
_sig("otti_k_sc_cubic3_fold_round", _i32, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _fp)
_sig("otti_k_poly_bound", _i32, _vp, _sz, _sz, _vp, _vp, _fp)
_sig("otti_k_bullet_round", _i32, _vp, _sz, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _fp)
_sig("otti_k_bullet_last_fold", _i32, _sz, _vp, _vp, _vp, _vp, _vp)
_u32 = ctypes.c_uint32
_sig("otti_k_fp_op", _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _fp)
_sig("otti_k_fr9_op", _i32, _i32, _vp, _vp, _vp, _sz, _vp, _vp, _fp)
_sig("otti_k_pt_op", _i32, _i32, _vp, _vp, _i32, _u32, _sz, _vp, _vp, _vp, _fp)
_sig("otti_k_pc_round", _i32, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _u32, _u32, _vp, _vp, _fp)
_sig("otti_k_pc_export", _i32, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp)
_sig("otti_k_pc_tail", _i32, _vp, _vp, _vp, _vp, _sz, _sz, _u32, _sz, _vp, _vp, _vp, _i32, _vp, _vp)
_sig("otti_k_prod_layer", _i32, _vp, _vp, _sz, _sz, _vp, _vp, _fp)
_sig("otti_k_hash_mem", _i32, _vp, _vp, _sz, _vp, _vp, _u32, _u32, _vp, _vp, _fp)
_sig("otti_k_hash_ops", _i32, _vp, _vp, _vp, _sz, _vp, _vp, _u32, _u32, _vp, _vp, _fp)
_sig("otti_k_pc_grid_cap_override", _i32, _vp)
_sig("otti_k_pc_plan", _i32, _sz, _sz, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_u64))
_sig("otti_k_dot_many", _i32, _vp, _vp, _sz, _sz, _vp, _fp)
_sig("otti_k_sum3", _i32, _vp, _vp, _vp, _sz, _sz, _vp, _fp)
_sig("otti_k_poly_bound_chunks", _i32, _vp, _sz, _sz, _vp, _sz, _vp, ctypes.POINTER(_i32), _fp)
_sig("otti_kd_multiply_vec", _i32, _vp, _vp, _vp, _vp, _vp, _vp)
_sig("otti_kd_check_sat", _i32, _vp, _vp, _vp, ctypes.POINTER(_u64), _vp)
_sig("otti_kd_eval_table_sparse", _i32, _vp, _vp, _vp, _vp, _vp)
_sig("otti_kd_eq_evals", _i32, _vp, _sz, _vp, _vp)
_sig("otti_kd_fold_top", _i32, _vp, _sz, _vp, _vp)
_sig("otti_kd_fold_bot", _i32, _vp, _vp, _sz, _vp, _vp)
_sig("otti_kd_sc_cubic_round", _i32, _vp, _vp, _vp, _vp, _sz, _vp, _vp)
_sig("otti_kd_sc_cubic_fold_round", _i32, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp)
_sig("otti_kd_sc_quad_round", _i32, _vp, _vp, _sz, _vp, _vp)
_sig("otti_kd_sc_quad_fold_round", _i32, _vp, _vp, _sz, _vp, _vp, _vp)
_sig("otti_kd_msm_rows", _i32, _vp, _vp, _sz, _sz, _vp, _vp, _vp)
_sig("otti_dev_alloc", _i32, _sz, ctypes.POINTER(_vp))
_sig("otti_dev_free", _i32, _vp)
_sig("otti_dev_upload", _i32, _vp, _vp, _sz)
_sig("otti_dev_download", _i32, _vp, _vp, _sz)
_sig("otti_dev_stream_create", _i32, ctypes.POINTER(_vp))
_sig("otti_dev_stream_sync", _i32, _vp)
_sig("otti_dev_stream_destroy", _i32, _vp)


def _last_error():
    buf = ctypes.create_string_buffer(512)
    lib.otti_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def _check(rc):
    if rc == 0:
        return
    msg = _last_error()
    if rc in (-10, -11, -12):
        raise ProofVerifyError(rc, msg)
    if rc == -20:
        raise NoDeviceError(rc, msg)
    if -6 <= rc <= -1:
        raise R1CSError(rc, msg)
    raise SpartanError(rc, msg)


def _ptr(a):
    return a.ctypes.data_as(_vp) if a is not None and a.size else None


def _scalars(a, what):
    """(n,32) uint8 array of canonical little-endian scalars"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 1:
        a = a.reshape(-1, 32)
    if a.ndim != 2 or a.shape[1] != 32:
        raise ValueError(f"{what}: expected an (n, 32) uint8 array")
    return a


def device_count():
    return int(lib.otti_device_count())


def host_selftest(iterations=200):
    """host-side fast paths of the prover (five-limb field, fixed-base tables) against the generic code; raises on a mismatch"""
    _check(lib.otti_host_selftest(iterations))


def host_point_from_uniform(b64):
    """a point (extended X, Y, Z, T: 128 bytes) from 64 uniform bytes"""
    assert len(b64) == 64
    out = ctypes.create_string_buffer(128)
    _check(lib.otti_host_point_from_uniform(bytes(b64), out))
    return out.raw


def host_point_sum(pts128, path, parts=1):
    """compressed sum of extended points (concatenated 128-byte records): path 0 generic code, 1 the prover's chunk-mail sum (IFMA where
    available), 2 the same in the scalar form, 3 as 1 with a stale last mail (raises)"""
    n = len(pts128) // 128
    out = ctypes.create_string_buffer(32)
    _check(lib.otti_host_point_sum(bytes(pts128), n, path, parts, out))
    return out.raw


def host_point_sum_bench(n=52, reps=2000):
    """nanoseconds per chunk mail summed on the host: (IFMA or 0, scalar)"""
    out = (ctypes.c_double * 2)()
    _check(lib.otti_host_point_sum_bench(n, reps, out))
    return out[0], out[1]


HOST_OPS = ("fixed_base_mul", "compress", "keccak_f1600", "append_point+challenge", "fr_mul", "fr_inv", "helper_thread_handoff",
            "zk_round_begin", "zk_round_finish", "threads")


def host_microbench():
    """nanoseconds per host-side primitive on this machine (no GPU needed); the last entry is the thread count used"""
    out = (ctypes.c_double * 10)()
    _check(lib.otti_host_microbench(out))
    return dict(zip(HOST_OPS, out))


def host_tail_bench(np_, nd, T, threads=1, reps=200):
    """microseconds per layer of SNARK mode's host-played sum-check rounds: {'avx512ifma': .., 'scalar': ..} (0 = form not available)"""
    out = (ctypes.c_double * 2)()
    _check(lib.otti_host_tail_bench(np_, nd, T, threads, reps, out))
    return {"avx512ifma": out[0], "scalar": out[1]}


# ---------------------------------------------------------------------------------------------- libspartan mirror
class Instance:
    """Instance::new(num_cons, num_vars, num_inputs, &A, &B, &C) -> Result<Instance, R1CSError>"""

    def __init__(self, handle, entries):
        self._h = handle
        self._keep = entries

    @classmethod
    def new(cls, num_cons, num_vars, num_inputs, A, B, C):
        ents = [np.ascontiguousarray(m, dtype=ENTRY_DTYPE) for m in (A, B, C)]
        h = _vp()
        _check(lib.otti_instance_new(num_cons, num_vars, num_inputs, _ptr(ents[0]), ents[0].size, _ptr(ents[1]), ents[1].size,
                                     _ptr(ents[2]), ents[2].size, ctypes.byref(h)))
        return cls(h, ents)

    @classmethod
    def from_zkif(cls, circuit, inputs, witness=None, mode="auto"):
        """otti_instance_from_zkif: the files to a ready instance in one call.  mode "host" is zkif_load + Instance.new; "device" parses the
        constraints on the GPU (the host lists exist only once something asks for them); "auto" takes the device when its runtime is up and the
        file's size allows.  Returns (Instance, assignment): the dict zkif_load returns, with A = B = C = None and their counts in nA, nB, nC."""
        enc = lambda s: None if s is None else os.fsencode(s)
        h, rp = _vp(), ctypes.POINTER(_R1CS)()
        _check(lib.otti_instance_from_zkif(enc(circuit), enc(inputs), enc(witness), INGEST_MODES[mode], ctypes.byref(h), ctypes.byref(rp)))
        counts = dict(nA=rp.contents.nA, nB=rp.contents.nB, nC=rp.contents.nC)
        assignment = _r1cs_to_py(rp)
        assignment.update(A=None, B=None, C=None, **counts)
        return cls(h, None), assignment

    @classmethod
    def from_coo(cls, num_cons, num_vars, num_inputs, A, B, C, stream=None, montgomery=False):
        """otti_instance_from_coo: the instance Instance.new makes from the same triples, from three arrays per matrix.  A, B, C: (rows, cols, vals)
        of numpy arrays or torch tensors.  rows / cols: int32, int64 (numpy also uint32, uint64), one dtype per matrix, made contiguous.  vals:
        int64 (negative: l - |x|) or uint64 numbers, or a uint8 array of shape (n, 32) of canonical scalars (``montgomery=True``: of Montgomery
        words); its stride along dimension 0 is passed on, so a strided view is read where it is.  Either all nine arrays live on the GPU or none
        does.  For GPU tensors ``stream`` defaults to torch's current stream (Witness.from_tensor's rule); torch has to be imported before
        otti_amd.  Validation runs on the device and raises what Instance.new raises for the same triples.  Nothing is kept
        alive once the call has returned."""
        mats = [tuple(m) for m in (A, B, C)]
        if any(len(m) != 3 for m in mats):
            raise ValueError("each matrix is (rows, cols, vals)")
        flat = [a for m in mats for a in m]
        torch = sys.modules.get("torch")
        on_gpu = [torch is not None and isinstance(a, torch.Tensor) and a.is_cuda for a in flat]
        if any(on_gpu) and not all(on_gpu):
            raise SpartanError(-21, "from_coo: either all nine arrays live on the GPU or none does")
        if all(on_gpu):
            coo, keep, producer = _coo_device(torch, mats, stream, montgomery)
        else:
            coo, keep, producer = _coo_host(torch, mats, montgomery), mats, None   # (mats: the contiguous forms the pointers go into)
        h = _vp()
        _check(lib.otti_instance_from_coo(num_cons, num_vars, num_inputs, coo, 1 if all(on_gpu) else 0, producer, ctypes.byref(h)))
        del keep
        return cls(h, None)

    def set_values(self, A=None, B=None, C=None, stream=None, montgomery=False):
        """otti_instance_set_values: new coefficients for the entries of A, B, C in place (None: that matrix stays).  Each is what from_coo takes
        as vals — 1-D int64 / uint64 or uint8 of shape (n, 32), numpy or torch, strided views read where they are — with one element per entry
        in ``entries`` order.  Either every array given lives on the GPU or none does; ``stream`` as in from_coo.  A coefficient >= l raises
        what Instance.new raises for the new triples and leaves the instance as it was.  Returns self."""
        given = [v for v in (A, B, C) if v is not None]
        torch = sys.modules.get("torch")
        on_gpu = [torch is not None and isinstance(v, torch.Tensor) and v.is_cuda for v in given]
        if any(on_gpu) and not all(on_gpu):
            raise SpartanError(-21, "set_values: either every array lives on the GPU or none does")
        dev = bool(on_gpu) and all(on_gpu)
        vals, keep, copied = (_CooValues * 3)(), [], False
        for k, v in enumerate((A, B, C)):
            if v is None:
                vals[k] = _CooValues(None, 0, WIT_CANONICAL32, 0)
                continue
            if dev:
                fmt = _coo_val_format(v.dtype == torch.int64 and v.dim() == 1, getattr(torch, "uint64", None) == v.dtype and v.dim() == 1,
                                      v.dtype == torch.uint8 and v.dim() == 2 and v.shape[1] == 32, montgomery)
                eb = 8 if fmt in (WIT_I64, WIT_U64) else 32
                n = v.shape[0]
                if n > 1 and (v.stride(0) * v.element_size() < eb or (v.dim() == 2 and v.stride(1) != 1)):
                    v, copied = v.contiguous(), True
                vals[k] = _CooValues(v.data_ptr() if v.numel() else None, n, fmt, v.stride(0) * v.element_size() if n > 1 else 0)
            else:
                v = v.numpy() if torch is not None and isinstance(v, torch.Tensor) else np.asarray(v)
                fmt = _coo_val_format(v.dtype == np.int64 and v.ndim == 1, v.dtype == np.uint64 and v.ndim == 1,
                                      v.dtype == np.uint8 and v.ndim == 2 and v.shape[1] == 32, montgomery)
                eb = 8 if fmt in (WIT_I64, WIT_U64) else 32
                n = v.shape[0]
                if n > 1 and (v.strides[0] < eb or (v.ndim == 2 and v.strides[1] != 1)):
                    v = np.ascontiguousarray(v)
                vals[k] = _CooValues(_ptr(v), n, fmt, v.strides[0] if n > 1 else 0)
            keep.append(v)                                     # alive until the call has returned
        producer = None
        if dev:
            if copied:                                         # a contiguous copy was queued on torch's current stream, whichever stream the caller names
                torch.cuda.current_stream(keep[0].device).synchronize()
            producer = _torch_stream(torch, keep[0], stream)
        _check(lib.otti_instance_set_values(self._h, vals, 1 if dev else 0, producer))
        del keep
        return self

    def values_info(self):
        """otti_instance_values_info: dict of generation (0 at creation, +1 per successful set_values), slots_resident and slot_bytes (the slot
        maps the first set_values of a device-ingested instance builds: 8 bytes per entry) and ms (staging, convert + validate, place) of the
        last call"""
        g, sr, sb, ms = _u64(), _i32(), _u64(), (ctypes.c_double * 3)()
        _check(lib.otti_instance_values_info(self._h, ctypes.byref(g), ctypes.byref(sr), ctypes.byref(sb), ms))
        return dict(generation=g.value, slots_resident=bool(sr.value), slot_bytes=sb.value, ms=tuple(ms))

    def values_kernel_ms(self):
        """otti_k_instance_values_kernel_ms: (convert, place) launches of the last set_values by HIP events, ms"""
        ms = (ctypes.c_float * 2)()
        _check(lib.otti_k_instance_values_kernel_ms(self._h, ms))
        return ms[0], ms[1]

    def device_entries(self, which):
        """otti_instance_device_entries: (ptr_row, ptr_col, ptr_val, n) of the entry lists a device-ingested instance keeps in HBM — u32 rows, u32
        padded columns, Montgomery values, caller order; (0, 0, 0, 0) for an instance that keeps none.  Valid while the instance lives."""
        r, c, v, n = _vp(), _vp(), _vp(), _sz()
        _check(lib.otti_instance_device_entries(self._h, which, ctypes.byref(r), ctypes.byref(c), ctypes.byref(v), ctypes.byref(n)))
        return r.value or 0, c.value or 0, v.value or 0, n.value

    def entries(self, which):
        """otti_instance_entries: the entries of A (0), B (1) or C (2) as the caller's — unpadded columns, canonical values, caller / file order"""
        n = _sz()
        _check(lib.otti_instance_entries(self._h, which, None, 0, ctypes.byref(n)))
        a = np.zeros(n.value, dtype=ENTRY_DTYPE)
        _check(lib.otti_instance_entries(self._h, which, _ptr(a) if n.value else None, n.value, ctypes.byref(n)))
        return a

    def ingest_info(self):
        """otti_instance_ingest_info: dict of on_device, circuit_bytes, hbm_entry_bytes and ms (host walk + id map, staging + copies, kernels, CSR build)"""
        on, cb, hb, ms = _i32(), _u64(), _u64(), (ctypes.c_double * 4)()
        _check(lib.otti_instance_ingest_info(self._h, ctypes.byref(on), ctypes.byref(cb), ctypes.byref(hb), ms))
        return dict(on_device=bool(on.value), circuit_bytes=cb.value, hbm_entry_bytes=hb.value, ms=tuple(ms))

    def host_lists_info(self):
        """otti_instance_host_lists_info: dict of materialised (the host entry lists exist: always for Instance.new; for a device ingest only once a
        host consumer has downloaded them) and host_bytes (their size, 0 while absent).  Asking never triggers the download."""
        m, hb = _i32(), _u64()
        _check(lib.otti_instance_host_lists_info(self._h, ctypes.byref(m), ctypes.byref(hb)))
        return dict(materialised=bool(m.value), host_bytes=hb.value)

    @property
    def dims(self):
        a, b, c = _u64(), _u64(), _u64()
        _check(lib.otti_instance_dims(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def is_sat(self, vars_, inputs):
        v, i = _scalars(vars_.assignment, "vars"), _scalars(inputs.assignment, "inputs")
        sat = _i32()
        _check(lib.otti_instance_is_sat(self._h, _ptr(v), v.shape[0], _ptr(i), i.shape[0], ctypes.byref(sat)))
        return bool(sat.value)

    def prepare_device(self, gens=None):
        _check(lib.otti_prepare_device(self._h, gens._h if gens is not None else None))

    def device_info(self, by_col=False):
        """which variants of the sparse kernels run on this instance (otti_instance_device_info): dict of rows, entries (A, B, C), use_small, quad,
        n_heavy, n_seg for the by-row copy (multiply_vec, check_sat) or the by-column one (eval_table_sparse)"""
        d = _DeviceInfo()
        _check(lib.otti_instance_device_info(self._h, 1 if by_col else 0, ctypes.byref(d)))
        return dict(rows=d.rows, entries=tuple(d.entries), use_small=bool(d.use_small), quad=bool(d.quad), n_heavy=d.n_heavy, n_seg=d.n_seg)

    def __del__(self):
        if getattr(self, "_h", None):
            lib.otti_instance_free(self._h)
            self._h = None


def _validate_scalars(a):
    # Scalar::from_bytes: canonical iff < l  (upstream returns Err(R1CSError::InvalidScalar))
    if a.shape[0] == 0:
        return
    words = a.view("<u8").reshape(-1, 4)
    lw = [(L_ORDER >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    bad = np.zeros(a.shape[0], dtype=bool)
    undecided = np.ones(a.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        gt = undecided & (words[:, k] > np.uint64(lw[k]))
        lt = undecided & (words[:, k] < np.uint64(lw[k]))
        bad |= gt
        undecided &= ~(gt | lt)
    bad |= undecided   # equal to l
    if bad.any():
        raise R1CSError(-5, "InvalidScalar")


class VarsAssignment:
    """VarsAssignment::new(&[[u8; 32]]) -> Result<_, R1CSError::InvalidScalar>"""

    def __init__(self, assignment):
        self.assignment = assignment

    @classmethod
    def new(cls, assignment):
        a = _scalars(assignment, "assignment")
        _validate_scalars(a)
        return cls(a)


class InputsAssignment(VarsAssignment):
    """InputsAssignment::new(&[[u8; 32]])"""


class NIZKGens:
    """NIZKGens::new(num_cons, num_vars, num_inputs)"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def new(cls, num_cons, num_vars, num_inputs):
        h = _vp()
        _check(lib.otti_gens_new(num_cons, num_vars, num_inputs, ctypes.byref(h)))
        return cls(h)

    @property
    def table_info(self):
        """(window bits, bytes) of the device-side fixed-base table; (0, 0) before it has been built"""
        c, b = ctypes.c_uint32(), _u64()
        _check(lib.otti_gens_table_info(self._h, ctypes.byref(c), ctypes.byref(b)))
        return c.value, b.value

    @property
    def build_ms(self):
        """(allocations, upload + kernels) of the last window-table build, in ms"""
        a, k = ctypes.c_double(), ctypes.c_double()
        _check(lib.otti_gens_build_ms(self._h, ctypes.byref(a), ctypes.byref(k)))
        return a.value, k.value

    def release_device(self):
        """free the device-side window table (rebuilt by the next prepare_device / proof)"""
        _check(lib.otti_gens_release_device(self._h))

    def adopt_table(self, donor):
        """drop this handle's device table and share ``donor``'s (built if need be); donor: NIZKGens of the same stream with at least as many points"""
        _check(lib.otti_gens_adopt_table(self._h, donor._h if donor is not None else None))

    def table_users(self):
        """(handles holding this handle's device table, its device address); (0, None) when there is none"""
        n, p = ctypes.c_uint32(), ctypes.c_void_p()
        _check(lib.otti_gens_table_users(self._h, ctypes.byref(n), ctypes.byref(p)))
        return n.value, p.value

    def points(self, count):
        out = np.zeros((count, 32), dtype=np.uint8)
        _check(lib.otti_gens_points(self._h, _ptr(out), count))
        return out

    def __del__(self):
        if getattr(self, "_h", None):
            lib.otti_gens_free(self._h)
            self._h = None


class SatReport:
    """What Witness.check_sat found: n_unsat failing constraints, the lowest of them in ``rows`` (uint64, ascending) and, when asked for,
    ``values[i]`` = canonical <A_r,z>, <B_r,z>, <C_r,z> of rows[i] as (3, 32) little-endian bytes.  True when the assignment satisfies."""

    def __init__(self, n_unsat, rows, values, kernel_ms):
        self.n_unsat, self.rows, self.values, self.kernel_ms = n_unsat, rows, values, kernel_ms

    def __bool__(self):
        return self.n_unsat == 0

    def __repr__(self):
        return f"SatReport(n_unsat={self.n_unsat}, rows={self.rows.tolist()})"


WIT_CANONICAL32, WIT_MONTGOMERY32, WIT_I64, WIT_U64 = 0, 1, 2, 3   # OTTI_WIT_*


def _dev_addr(p):
    return p.ptr if hasattr(p, "ptr") else p


def _int_array(a):
    a = np.asarray(a)
    if a.dtype not in (np.int64, np.uint64) or a.ndim != 1:
        raise ValueError("expected a 1-D numpy array of int64 or uint64")
    return np.ascontiguousarray(a), WIT_I64 if a.dtype == np.int64 else WIT_U64


def _host_values(a):
    """(contiguous array, WIT_*) of host values Witness.update / scatter take: int64 / uint64 numbers, else (n, 32) uint8 canonical scalars"""
    if a.dtype in (np.int64, np.uint64):
        return _int_array(a)
    return _scalars(a, "values"), WIT_CANONICAL32


def _torch_if(*objs):
    """the torch module when every one of objs is a torch tensor, else None.  A tensor that came in has its module loaded: torch is never
    imported here (from_tensor alone does that)"""
    torch = sys.modules.get("torch")
    return torch if torch is not None and all(isinstance(o, torch.Tensor) for o in objs) else None


def _tensor_layout(torch, t):
    """(format, count, stride_bytes) of a GPU tensor Witness.from_tensor / update take"""
    if not t.is_cuda:
        raise ValueError("expected a tensor on the GPU")
    if t.dtype == torch.int64 and t.dim() == 1:
        if t.shape[0] > 1 and t.stride(0) < 1:
            raise ValueError("an int64 tensor needs a positive stride")
        return WIT_I64, t.shape[0], t.stride(0) * 8 if t.shape[0] > 1 else 0
    if t.dtype == torch.uint8 and t.dim() == 2 and t.shape[1] == 32 and t.is_contiguous():
        return WIT_CANONICAL32, t.shape[0], 0
    raise ValueError("expected a 1-D int64 tensor or a contiguous uint8 tensor of shape (n, 32)")


def _torch_stream(torch, t, stream):
    """the hipStream_t to order an ingest of tensor t after: the given one, else torch's current stream on t's device.  torch's default stream
    is HIP's null stream, handle 0, which the C ABI reads as "no stream to wait for" and the library's non-blocking stream is not ordered
    against: its pending work is waited for here, on the host"""
    if stream is not None:
        return stream
    cur = torch.cuda.current_stream(t.device)
    if not cur.cuda_stream:
        cur.synchronize()
        return None
    return cur.cuda_stream


_NP_INDEX = {np.dtype(np.uint32): IDX_U32, np.dtype(np.int32): IDX_I32, np.dtype(np.uint64): IDX_U64, np.dtype(np.int64): IDX_I64}


def _coo_val_format(is_int64, is_uint64, is_bytes32, montgomery):
    if is_int64 or is_uint64:
        if montgomery:
            raise ValueError("montgomery=True goes with (n, 32) uint8 coefficients")
        return WIT_I64 if is_int64 else WIT_U64
    if is_bytes32:
        return WIT_MONTGOMERY32 if montgomery else WIT_CANONICAL32
    raise ValueError("coefficients: expected 1-D int64 / uint64 or uint8 of shape (n, 32)")


def _coo_host(torch, mats, montgomery):
    """Instance.from_coo's otti_coo[3] over host arrays (numpy, or torch tensors on the CPU, whose memory numpy views)"""
    coo = (_Coo * 3)()
    for k, m in enumerate(mats):
        rows, cols, vals = (a.numpy() if torch is not None and isinstance(a, torch.Tensor) else np.asarray(a) for a in m)
        if rows.dtype != cols.dtype or rows.dtype not in _NP_INDEX or rows.ndim != 1 or cols.ndim != 1:
            raise ValueError("rows and cols: two 1-D arrays of one dtype among int32, int64, uint32, uint64")
        rows, cols = np.ascontiguousarray(rows), np.ascontiguousarray(cols)
        fmt = _coo_val_format(vals.dtype == np.int64 and vals.ndim == 1, vals.dtype == np.uint64 and vals.ndim == 1,
                              vals.dtype == np.uint8 and vals.ndim == 2 and vals.shape[1] == 32, montgomery)
        n = vals.shape[0]
        if rows.shape[0] != n or cols.shape[0] != n:
            raise ValueError("rows, cols and vals of one matrix have one length")
        eb = 8 if fmt in (WIT_I64, WIT_U64) else 32
        if n > 1 and (vals.strides[0] < eb or (vals.ndim == 2 and vals.strides[1] != 1)):
            vals = np.ascontiguousarray(vals)                 # (a reversed or overlapping view; an odd stride is the library's to refuse)
        coo[k] = _Coo(_ptr(rows), _ptr(cols), _ptr(vals), n, _NP_INDEX[rows.dtype], fmt, vals.strides[0] if n > 1 else 0)
        mats[k] = (rows, cols, vals)                           # alive until the call has returned
    return coo


def _coo_device(torch, mats, stream, montgomery):
    """Instance.from_coo's otti_coo[3] over GPU tensors, the tensors it points into and the stream to order the ingest after"""
    index = {torch.int32: IDX_I32, torch.int64: IDX_I64}
    for name, fmt in (("uint32", IDX_U32), ("uint64", IDX_U64)):
        if hasattr(torch, name):
            index[getattr(torch, name)] = fmt
    coo, keep, copied = (_Coo * 3)(), [], False
    for k, (rows, cols, vals) in enumerate(mats):
        if rows.dtype != cols.dtype or rows.dtype not in index or rows.dim() != 1 or cols.dim() != 1:
            raise ValueError("rows and cols: two 1-D tensors of one dtype among int32, int64")
        fmt = _coo_val_format(vals.dtype == torch.int64 and vals.dim() == 1, getattr(torch, "uint64", None) == vals.dtype and vals.dim() == 1,
                              vals.dtype == torch.uint8 and vals.dim() == 2 and vals.shape[1] == 32, montgomery)
        n = vals.shape[0]
        if rows.shape[0] != n or cols.shape[0] != n:
            raise ValueError("rows, cols and vals of one matrix have one length")
        eb = 8 if fmt in (WIT_I64, WIT_U64) else 32
        fixed = [rows.contiguous(), cols.contiguous(), vals]
        if n > 1 and (vals.stride(0) * vals.element_size() < eb or (vals.dim() == 2 and vals.stride(1) != 1)):
            fixed[2] = vals.contiguous()
        copied = copied or any(a is not b for a, b in zip(fixed, (rows, cols, vals)))
        rows, cols, vals = fixed
        keep.append(fixed)
        p = lambda t: t.data_ptr() if t.numel() else None
        coo[k] = _Coo(p(rows), p(cols), p(vals), n, index[rows.dtype], fmt, vals.stride(0) * vals.element_size() if n > 1 else 0)
    if copied:                                                 # a contiguous copy was queued on torch's current stream, whichever stream the caller names
        torch.cuda.current_stream(mats[0][2].device).synchronize()
    return coo, keep, _torch_stream(torch, mats[0][2], stream)


class Witness:
    """Assignment resident in HBM (z = vars || 1 || inputs || 0..): upload once, prove many times."""

    def __init__(self, inst, vars_, inputs):
        v, i = _scalars(vars_.assignment, "vars"), _scalars(inputs.assignment, "inputs")
        h = _vp()
        _check(lib.otti_witness_upload(inst._h, _ptr(v), v.shape[0], _ptr(i), i.shape[0], ctypes.byref(h)))
        self._h = h

    @classmethod
    def _adopt(cls, handle):
        w = cls.__new__(cls)
        w._h = handle
        return w

    @classmethod
    def from_device(cls, inst, ptr, nvars, fmt, inputs, stride_bytes=0, stream=None):
        """From ``nvars`` elements in device memory at address ``ptr`` (an int or a DeviceArray) in format ``fmt`` (WIT_*), ``stride_bytes`` apart
        (0: packed); ``stream``: the hipStream_t whose queued work writes them (otti_witness_from_device)."""
        i = _scalars(inputs.assignment, "inputs")
        h = _vp()
        _check(lib.otti_witness_from_device(inst._h, _dev_addr(ptr), nvars, fmt, stride_bytes, _ptr(i), i.shape[0], stream, ctypes.byref(h)))
        return cls._adopt(h)

    @classmethod
    def from_ints(cls, inst, array, inputs):
        """From a host numpy array of int64 (WIT_I64) or uint64 (WIT_U64): 8 bytes per variable cross PCIe (otti_witness_upload_ints)"""
        a, fmt = _int_array(array)
        i = _scalars(inputs.assignment, "inputs")
        h = _vp()
        _check(lib.otti_witness_upload_ints(inst._h, _ptr(a), a.size, fmt, _ptr(i), i.shape[0], ctypes.byref(h)))
        return cls._adopt(h)

    @classmethod
    def from_tensor(cls, inst, tensor, inputs, stream=None):
        """From a torch tensor on the GPU: 1-D int64 (contiguous or a strided view) as WIT_I64, uint8 of shape (n, 32) as WIT_CANONICAL32.
        ``stream`` defaults to torch's current stream, whose queued work is waited for on the device; when that is torch's default stream
        (HIP's null stream, which the C ABI cannot name) it is synchronised on the host instead.  torch has to be imported before otti_amd
        so that both use one HIP runtime."""
        import torch
        fmt, nvars, stride = _tensor_layout(torch, tensor)
        return cls.from_device(inst, tensor.data_ptr(), nvars, fmt, inputs, stride, _torch_stream(torch, tensor, stream))

    @classmethod
    def from_zkif(cls, inst, inputs, witness, mode="auto"):
        """otti_witness_from_zkif: the .inp.zkif and .wit.zkif files to a resident witness of ``inst``, equal to zkif_load + upload.  mode "host"
        parses the two files on the host and uploads; "device" ships the Witness messages to HBM and reads them there; "auto" takes the device
        from OTTI_INGEST_WIT_MIN_MB MiB of witness file on.  A defective file raises what zkif_load + Witness raise for it.  Returns
        (Witness, public inputs as an (n, 32) uint8 array)."""
        h, rp = _vp(), ctypes.POINTER(_R1CS)()
        _check(lib.otti_witness_from_zkif(inst._h, os.fsencode(inputs), os.fsencode(witness), INGEST_MODES[mode], ctypes.byref(h), ctypes.byref(rp)))
        return cls._adopt(h), _r1cs_to_py(rp)["inputs"]

    def ingest_info(self):
        """otti_witness_ingest_info: dict of on_device, witness_bytes and ms (host walk, staging + copies, kernel)"""
        on, wb, ms = _i32(), _u64(), (ctypes.c_double * 3)()
        _check(lib.otti_witness_ingest_info(self._h, ctypes.byref(on), ctypes.byref(wb), ms))
        return dict(on_device=bool(on.value), witness_bytes=wb.value, ms=tuple(ms))

    def _source(self, values, fmt, stride_bytes, stream, what):
        """(src, count, fmt, stride_bytes, on_device, stream, keep-alive) of the ``values`` update / assign / diff take"""
        if isinstance(values, tuple):
            if fmt is None:
                raise ValueError(f"{what} from a device address needs fmt")
            return _dev_addr(values[0]), values[1], fmt, stride_bytes, 1, stream, values
        if isinstance(values, np.ndarray):
            keep, f = _host_values(values)
            return _ptr(keep), keep.shape[0], f if fmt is None else fmt, 0, 0, stream, keep
        torch = _torch_if(values)
        if torch is None:
            raise ValueError("values: expected a numpy int64 / uint64 array, an (n, 32) uint8 numpy array, a torch GPU tensor or (address, count)")
        f, count, stride_bytes = _tensor_layout(torch, values)
        return values.data_ptr(), count, f if fmt is None else fmt, stride_bytes, 1, _torch_stream(torch, values, stream), values

    def update(self, inst, first, values, fmt=None, stride_bytes=0, stream=None):
        """Replace variables [first, first + count) in place (otti_witness_update).  ``values``: a numpy int64 / uint64 array or (n, 32) uint8
        canonical scalars on the host; a torch GPU tensor (as from_tensor); or ``(address, count)`` of device memory with ``fmt`` given.
        A scalar >= l raises R1CSError(-5) and leaves the witness as it was."""
        src, count, fmt, stride_bytes, on_device, stream, _keep = self._source(values, fmt, stride_bytes, stream, "update")
        _check(lib.otti_witness_update(inst._h, self._h, first, src, count, fmt, stride_bytes, on_device, stream))

    def assign(self, inst, values, first=0, fmt=None, stride_bytes=0, stream=None):
        """Set variables [first, first + count) from a whole new vector of which most elements usually have not moved (otti_witness_assign):
        the vector is compared with the resident one on the device, by value, only the changed elements are written and kept rows are brought
        up to date by the changes alone.  ``values`` as update takes them.  Returns the number of changed elements.  A scalar >= l raises
        R1CSError(-5) and leaves the witness as it was."""
        src, count, fmt, stride_bytes, on_device, stream, _keep = self._source(values, fmt, stride_bytes, stream, "assign")
        n = _u64()
        _check(lib.otti_witness_assign(inst._h, self._h, first, src, count, fmt, stride_bytes, on_device, stream, ctypes.byref(n)))
        return n.value

    def diff(self, inst, values, first=0, fmt=None, stride_bytes=0, stream=None, max_indices=64):
        """What assign would change, without changing it (otti_witness_diff): (n_changed, the lowest min(n_changed, max_indices) changed
        indices as an ascending uint64 array)."""
        src, count, fmt, stride_bytes, on_device, stream, _keep = self._source(values, fmt, stride_bytes, stream, "diff")
        n, idx = _u64(), np.zeros(max_indices, dtype=np.uint64)
        _check(lib.otti_witness_diff(inst._h, self._h, first, src, count, fmt, stride_bytes, on_device, stream, ctypes.byref(n), _ptr(idx), max_indices))
        return n.value, idx[:min(n.value, max_indices)].copy()

    def assign_info(self):
        """(calls, changed, resums): assign calls that were not refused, elements they changed, calls that summed kept rows again instead of patching them"""
        a, b, c = _u64(), _u64(), _u64()
        _check(lib.otti_witness_assign_info(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def scatter(self, inst, indices, values, fmt=None, stream=None):
        """Replace the variables ``indices`` by ``values`` in place (otti_witness_scatter); kept rows are patched by the changes, not summed again.
        ``indices``: a numpy int64 / uint64 array with ``values`` a numpy int64 / uint64 array or (n, 32) uint8 canonical scalars (``fmt`` names
        another 32-byte format); or both torch GPU tensors, int64 indices and values as from_tensor takes them.  Indices in any order are sorted
        here, the values alongside; a duplicate or negative index raises ValueError before the library is called.  A scalar >= l raises
        R1CSError(-5), an index beyond the variables R1CSError(-6), and either leaves the witness as it was."""
        if isinstance(indices, np.ndarray) or isinstance(indices, (list, tuple)):
            idx = np.asarray(indices)
            if idx.ndim != 1 or idx.dtype not in (np.int64, np.uint64):
                raise ValueError("indices: expected a 1-D numpy array of int64 or uint64")
            if idx.dtype == np.int64 and idx.size and int(idx.min()) < 0:
                raise ValueError("indices: a negative index")
            idx = idx.astype(np.uint64)
            if not isinstance(values, np.ndarray):
                raise ValueError("values: host indices go with a numpy int64 / uint64 array or (n, 32) uint8 canonical scalars")
            vals, f = _host_values(values)
            if vals.shape[0] != idx.size:
                raise ValueError("indices and values differ in length")
            if idx.size > 1 and not bool(np.all(idx[1:] > idx[:-1])):
                order = np.argsort(idx, kind="stable")
                idx, vals = np.ascontiguousarray(idx[order]), np.ascontiguousarray(vals[order])
                if not bool(np.all(idx[1:] > idx[:-1])):
                    raise ValueError("indices: an index occurs twice")
            idx = np.ascontiguousarray(idx)
            fmt = f if fmt is None else fmt
            _check(lib.otti_witness_scatter(inst._h, self._h, _ptr(idx), _ptr(vals), idx.size, fmt, 0, 0, None))
            return
        torch = _torch_if(indices, values)
        if torch is None:
            raise ValueError("indices / values: expected numpy arrays, or torch GPU tensors for both")
        if not indices.is_cuda or indices.dtype != torch.int64 or indices.dim() != 1:
            raise ValueError("indices: expected a 1-D int64 tensor on the GPU")
        f, count, stride = _tensor_layout(torch, values)
        if count != indices.shape[0]:
            raise ValueError("indices and values differ in length")
        fmt = f if fmt is None else fmt
        if stream is not None:
            ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=indices.device))
        else:
            ctx = contextlib.nullcontext()
        with ctx:                                                  # the checks and the sort run where the tensors were produced
            if count and bool((indices < 0).any()):
                raise ValueError("indices: a negative index")
            if count > 1 and not bool((indices[1:] > indices[:-1]).all()):
                indices, order = torch.sort(indices)
                values = values.index_select(0, order)
                stride = 0
                if bool((indices[1:] == indices[:-1]).any()):
                    raise ValueError("indices: an index occurs twice")
            indices = indices.contiguous()
            stream = _torch_stream(torch, indices, stream)
        _check(lib.otti_witness_scatter(inst._h, self._h, indices.data_ptr(), values.data_ptr(), count, fmt, stride, 1, stream))

    def scatter_info(self):
        """(calls, rows_patched, terms_patched): scatter calls that changed the witness, kept rows patched by them, (index, delta) terms summed into kept rows"""
        a, b, c = _u64(), _u64(), _u64()
        _check(lib.otti_witness_scatter_info(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def set_inputs(self, inst, inputs):
        """Replace the public inputs of the resident witness (otti_witness_set_inputs); ``inputs``: InputsAssignment or (n, 32) uint8 canonical
        scalars.  Kept rows cover the variables alone and stay valid."""
        i = _scalars(inputs.assignment if hasattr(inputs, "assignment") else inputs, "inputs")
        _check(lib.otti_witness_set_inputs(inst._h, self._h, _ptr(i), i.shape[0]))

    @property
    def info(self):
        """(device address of z, its length n = 2 * padded num_vars Montgomery elements, small_fraction)"""
        p, n, f = _vp(), _sz(), ctypes.c_double()
        _check(lib.otti_witness_info(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(f)))
        return p.value, n.value, f.value

    def keep_rows(self, inst, gens):
        """Sum the commitment's unblinded rows now and keep them with the witness (otti_witness_keep_rows[_snark]); ``gens``: NIZKGens or
        SNARKGens.  Proofs over the same generator points, NIZK and SNARK alike, then skip the commitment's large MSM launch, and ``update`` sums only the
        rows it touches again.  Proof bytes do not change.  Costs 128 * L bytes of HBM."""
        f = lib.otti_witness_keep_rows_snark if isinstance(gens, SNARKGens) else lib.otti_witness_keep_rows
        _check(f(inst._h, self._h, gens._h))
        self._rows_gens = gens                                    # updates sum rows over this handle's table: it outlives the kept rows

    def drop_rows(self):
        """Free the kept rows (otti_witness_drop_rows); the witness then proves as one that never kept them"""
        _check(lib.otti_witness_drop_rows(self._h))
        self._rows_gens = None

    def rows_info(self):
        """(kept, L, R, rows_resummed): whether rows are kept, their geometry, and how many rows updates have summed again since keep_rows"""
        k, L, R, n = _i32(), _sz(), _sz(), _u64()
        _check(lib.otti_witness_rows_info(self._h, ctypes.byref(k), ctypes.byref(L), ctypes.byref(R), ctypes.byref(n)))
        return bool(k.value), L.value, R.value, n.value

    def keep_products(self, inst):
        """Form Az, Bz, Cz, the verdict bitmap and the failing count of this assignment over ``inst`` now and keep them with the witness
        (otti_witness_keep_products).  Every mutator then recomputes only the rows its changed variables reach; proofs over ``inst`` copy the
        vectors instead of forming them and check_sat answers without a pass.  Proof bytes do not change.  Costs 96 * N + N / 8 bytes of HBM."""
        _check(lib.otti_witness_keep_products(inst._h, self._h))
        self._products_inst = inst                                # the patches read this instance's matrices: it outlives the kept products

    def drop_products(self):
        """Free the kept products (otti_witness_drop_products); the witness then proves and checks as one that never kept them"""
        _check(lib.otti_witness_drop_products(self._h))
        self._products_inst = None

    def products_info(self):
        """dict(kept, n_rows, d_Az, d_Bz, d_Cz, n_unsat, patches, rows_recomputed, full_passes) (otti_witness_products_info); the three device
        addresses are read-only and None when nothing is kept"""
        k, n = _i32(), _sz()
        a, b, c = _vp(), _vp(), _vp()
        u, pt, rr, fp = _u64(), _u64(), _u64(), _u64()
        _check(lib.otti_witness_products_info(self._h, ctypes.byref(k), ctypes.byref(n), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                              ctypes.byref(u), ctypes.byref(pt), ctypes.byref(rr), ctypes.byref(fp)))
        return dict(kept=bool(k.value), n_rows=n.value, d_Az=a.value, d_Bz=b.value, d_Cz=c.value, n_unsat=u.value, patches=pt.value,
                    rows_recomputed=rr.value, full_passes=fp.value)

    def check_sat(self, inst, max_rows=64, values=True):
        """Instance::is_sat on the device, on this resident assignment, with the failing constraints named (otti_witness_check_sat)"""
        n, ms = _u64(), ctypes.c_float()
        rows = np.zeros(max_rows, dtype=np.uint64)
        abc = np.zeros((max_rows, 3, 32), dtype=np.uint8) if values else None
        _check(lib.otti_witness_check_sat(inst._h, self._h, ctypes.byref(n), _ptr(rows), max_rows, _ptr(abc), ctypes.byref(ms)))
        k = min(n.value, max_rows)
        return SatReport(n.value, rows[:k].copy(), abc[:k].copy() if values else None, ms.value)

    def __del__(self):
        if getattr(self, "_h", None):
            lib.otti_witness_free(self._h)
            self._h = None


STAGES = ("polycommit", "multiply_vec", "sc_phase_one", "eval_table_sparse", "sc_phase_two", "polyeval", "total")


class NIZK:
    """NIZK::prove(&inst, vars, &inputs, &gens, &mut Transcript::new(label)) / NIZK::verify(...)"""

    def __init__(self, proof_bytes, stage_ms=None):
        self.bytes = proof_bytes
        self.stage_ms = stage_ms

    @staticmethod
    def _take(ptr, n):
        data = ctypes.string_at(ptr, n.value)
        lib.otti_buf_free(ptr)
        return data

    @classmethod
    def prove(cls, inst, vars_, inputs, gens, transcript_label=b"nizk_example", seed=None):
        label = bytes(transcript_label)
        if isinstance(vars_, Witness):
            w = vars_
            p, n, ms = _vp(), _sz(), (ctypes.c_double * 8)()
            _check(lib.otti_nizk_prove_resident(inst._h, w._h, gens._h, label, len(label), _seed(seed), ctypes.byref(p), ctypes.byref(n), ms))
            return cls(cls._take(p, n), dict(zip(STAGES, ms)))
        v, i = _scalars(vars_.assignment, "vars"), _scalars(inputs.assignment, "inputs")
        p, n, ms = _vp(), _sz(), (ctypes.c_double * 8)()
        _check(lib.otti_nizk_prove(inst._h, _ptr(v), v.shape[0], _ptr(i), i.shape[0], gens._h, label, len(label), _seed(seed), 1,
                                   ctypes.byref(p), ctypes.byref(n), ms))
        return cls(cls._take(p, n), dict(zip(STAGES, ms)))

    @classmethod
    def prove_many(cls, inst, witnesses, gens, transcript_label=b"nizk_example", seeds=None, threads=0, details=False):
        """Many resident witnesses of ONE instance proved in one call (otti_nizk_prove_many): the witness-only work of the proofs — commitment row
        sums, Az, Bz, Cz — is formed for the batch in joint passes, the library's own ``threads`` workers (0 = its default, 4; at most 16; the
        calling thread counts) run the rest.  ``seeds``: None, or one 32-byte seed or None per witness.  Returns a list of NIZK objects — element k
        has the bytes ``prove(inst, witnesses[k], .., seed=seeds[k])`` gives — with None where an item failed, which raises nothing; only the call's
        own refusals raise.  ``details=True``: (proofs, result codes, info dict) as well.  The handles are only read; one may appear several times."""
        label = bytes(transcript_label)
        wits = list(witnesses)
        n = len(wits)
        per = list(seeds) if seeds is not None else [None] * n
        if len(per) != n:
            raise ValueError("prove_many: one seed (or None) per witness")
        hs, sd = (_vp * max(1, n))(), (_vp * max(1, n))()
        keep = [_seed(x) for x in per]                            # the seed buffers live until the call returns
        for k in range(n):
            hs[k], sd[k] = wits[k]._h, keep[k]
        pf, lens, res = (_vp * max(1, n))(), (_sz * max(1, n))(), (_i32 * max(1, n))()
        failed, ms, info = _sz(0), (ctypes.c_double * (8 * max(1, n)))(), _ProveManyInfo()
        _check(lib.otti_nizk_prove_many(inst._h, hs, n, gens._h, label, len(label), sd, threads, pf, lens, res, ctypes.byref(failed), ms, ctypes.byref(info)))
        out = []
        for k in range(n):
            if res[k] == 0:
                data = ctypes.string_at(pf[k], lens[k])
                lib.otti_buf_free(pf[k])
                out.append(cls(data, dict(zip(STAGES, ms[8 * k:8 * k + 8]))))
            else:
                assert not pf[k]
                out.append(None)
        codes = [int(res[k]) for k in range(n)]
        assert failed.value == sum(1 for r in codes if r != 0)
        return (out, codes, info.as_dict()) if details else out

    @classmethod
    def prove_sharded(cls, inst, witness, gens, transcript_label=b"nizk_example", seed=None):
        """This rank's part of ONE proof spread over the GPUs of a node (collective over the ranks of ``shard_init``; every rank
        passes the same instance, resident witness, generators, label and 32-byte seed and gets the same proof bytes back)."""
        label = bytes(transcript_label)
        p, n, ms = _vp(), _sz(), (ctypes.c_double * 8)()
        _check(lib.otti_nizk_prove_sharded(inst._h, witness._h, gens._h, label, len(label), _seed(seed), ctypes.byref(p), ctypes.byref(n), ms))
        return cls(cls._take(p, n), dict(zip(STAGES, ms)))

    def verify(self, inst, inputs, gens, transcript_label=b"nizk_example"):
        """Ok(()) -> None; Err(ProofVerifyError) -> raises"""
        label = bytes(transcript_label)
        i = _scalars(inputs.assignment, "inputs")
        buf = np.frombuffer(self.bytes, dtype=np.uint8)
        _check(lib.otti_nizk_verify(inst._h, _ptr(i), i.shape[0], gens._h, label, len(label), _ptr(buf), buf.size))

    @staticmethod
    def verify_many(inst, proofs, inputs, gens, transcript_label=b"nizk_example", threads=0):
        """Many proofs of ONE instance in one call (otti_nizk_verify_many): ``proofs`` are NIZK objects or bytes, ``inputs`` one InputsAssignment for
        all of them or one per proof.  Returns the list of result codes — element i is what ``verify`` on proof i alone would report, 0 = accepted —
        so a rejected proof raises nothing; only the call's own refusals (bad arguments) raise.  Not a randomised batch: no verdict depends on
        another proof.  ``threads``: the library's worker threads, 0 = its default, at most 16; the call blocks until all are done."""
        label = bytes(transcript_label)
        blobs = [np.frombuffer(bytes(p.bytes if isinstance(p, NIZK) else p), dtype=np.uint8) for p in proofs]
        n = len(blobs)
        per = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs] * n
        if len(per) != n:
            raise ValueError("verify_many: one InputsAssignment for all proofs, or one per proof")
        ins = [_scalars(i.assignment, "inputs") for i in per]
        in_ptrs, in_counts = (_vp * max(1, n))(), (_sz * max(1, n))()
        pf_ptrs, pf_lens = (_vp * max(1, n))(), (_sz * max(1, n))()
        empty = np.zeros(1, dtype=np.uint8)
        for k in range(n):
            in_ptrs[k], in_counts[k] = _ptr(ins[k]), ins[k].shape[0]
            pf_ptrs[k], pf_lens[k] = (blobs[k] if blobs[k].size else empty).ctypes.data_as(_vp), blobs[k].size   # an empty proof is a malformed one, not a null pointer
        results, rejected = (_i32 * max(1, n))(), _sz(0)
        _check(lib.otti_nizk_verify_many(inst._h, gens._h, label, len(label), n, in_ptrs, in_counts, pf_ptrs, pf_lens, threads, results, ctypes.byref(rejected)))
        out = [int(results[k]) for k in range(n)]
        assert rejected.value == sum(1 for r in out if r != 0)
        return out

    @staticmethod
    def verify_batch(inst, proofs, inputs, gens, transcript_label=b"nizk_example", threads=0, seed=None, details=False):
        """Many proofs of ONE instance as one randomised batch (otti_nizk_verify_batch): the arguments and the returned list of codes are
        ``verify_many``'s — element i is what ``verify`` on proof i alone would report, except that a proof it rejects is accepted with
        probability at most 2^-120 over the library's randomness.  ``seed`` (32 bytes) repeats a run in tests; a seed the prover could know
        forfeits soundness, so leave it None.  ``details=True`` returns (codes, info dict: the otti_verify_batch_info counters)."""
        label = bytes(transcript_label)
        blobs = [np.frombuffer(bytes(p.bytes if isinstance(p, NIZK) else p), dtype=np.uint8) for p in proofs]
        n = len(blobs)
        per = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs] * n
        if len(per) != n:
            raise ValueError("verify_batch: one InputsAssignment for all proofs, or one per proof")
        ins = [_scalars(i.assignment, "inputs") for i in per]
        in_ptrs, in_counts = (_vp * max(1, n))(), (_sz * max(1, n))()
        pf_ptrs, pf_lens = (_vp * max(1, n))(), (_sz * max(1, n))()
        empty = np.zeros(1, dtype=np.uint8)
        for k in range(n):
            in_ptrs[k], in_counts[k] = _ptr(ins[k]), ins[k].shape[0]
            pf_ptrs[k], pf_lens[k] = (blobs[k] if blobs[k].size else empty).ctypes.data_as(_vp), blobs[k].size
        results, rejected, info = (_i32 * max(1, n))(), _sz(0), _VerifyBatchInfo()
        _check(lib.otti_nizk_verify_batch(inst._h, gens._h, label, len(label), n, in_ptrs, in_counts, pf_ptrs, pf_lens, threads, _seed(seed), results,
                                          ctypes.byref(rejected), ctypes.byref(info)))
        out = [int(results[k]) for k in range(n)]
        assert rejected.value == sum(1 for r in out if r != 0)
        if not details:
            return out
        return out, {k: getattr(info, k) for k, _ in _VerifyBatchInfo._fields_ }


# ---------------------------------------------------------------------------------------------- SNARK mode (lib.rs SNARKGens / SNARK)
class SNARKGens:
    """SNARKGens::new(num_cons, num_vars, num_inputs, num_nz_entries)"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def new(cls, num_cons, num_vars, num_inputs, num_nz_entries):
        h = _vp()
        _check(lib.otti_snark_gens_new(num_cons, num_vars, num_inputs, num_nz_entries, ctypes.byref(h)))
        return cls(h)

    def points(self, which):
        """the generator stream "sat" (gens_r1cs_sat) or "eval" (gens_r1cs_eval) as an (n, 32) array of compressed points"""
        w, n = {"sat": 0, "eval": 1}[which], _sz()
        _check(lib.otti_snark_gens_points(self._h, w, None, 0, ctypes.byref(n)))
        out = np.zeros((n.value, 32), dtype=np.uint8)
        _check(lib.otti_snark_gens_points(self._h, w, _ptr(out), n.value, ctypes.byref(n)))
        return out

    def __del__(self):
        if getattr(self, "_h", None):
            lib.otti_snark_gens_free(self._h)
            self._h = None


class ComputationCommitment:
    """SNARK::encode(&inst, &gens) -> (ComputationCommitment, ComputationDecommitment); `from_bytes` gives the verifier's copy, which
    `attach` completes into a prover's copy (the decommitment is rebuilt from the instance on the device, never stored)"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def encode(cls, inst, gens):
        h = _vp()
        _check(lib.otti_snark_encode(inst._h, gens._h, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def from_bytes(cls, data):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        h = _vp()
        _check(lib.otti_comp_comm_from_bytes(_ptr(buf), buf.size, ctypes.byref(h)))
        return cls(h)

    @property
    def bytes(self):
        p, n = _vp(), _sz()
        _check(lib.otti_comp_comm_bytes(self._h, ctypes.byref(p), ctypes.byref(n)))
        return NIZK._take(p, n)

    def attach(self, inst, gens, verify=False):
        """Rebuild the decommitment of ``inst`` on the device.  ``verify``: also recompute both commitments and compare them with the
        stored points (raises SpartanError, code -21, on a difference); without it the caller is trusted beyond the dimensions."""
        _check(lib.otti_comp_comm_attach(self._h, inst._h, gens._h, 1 if verify else 0))
        return self

    def revalue(self, inst, gens):
        """otti_comp_comm_revalue: this commitment (with its decommitment) brought to ``inst``'s current coefficients after Instance.set_values:
        only the values and the commitment rows that hold them are computed again; ``bytes`` then equals a fresh encode's."""
        _check(lib.otti_comp_comm_revalue(self._h, inst._h, gens._h))
        return self

    def _dims(self):
        nc, nv, ni, no, has = _u64(), _u64(), _u64(), _u64(), _i32()
        _check(lib.otti_comp_comm_dims(self._h, ctypes.byref(nc), ctypes.byref(nv), ctypes.byref(ni), ctypes.byref(no), ctypes.byref(has)))
        return (nc.value, nv.value, ni.value, no.value), bool(has.value)

    @property
    def dims(self):
        """(num_cons, num_vars, num_inputs, num_ops): SNARKGens.new(*dims) gives the encoder's generators"""
        return self._dims()[0]

    @property
    def has_decommitment(self):
        return self._dims()[1]

    def __del__(self):
        if getattr(self, "_h", None):
            lib.otti_comp_comm_free(self._h)
            self._h = None


SNARK_STAGES = ("polycommit", "multiply_vec", "sc_phase_one", "eval_table_sparse", "sc_phase_two", "polyeval", "derefs_commit", "product_circuits", "hash_layer", "total")


class SNARK:
    """SNARK::prove(&inst, &comm, &decomm, vars, &inputs, &gens, &mut Transcript::new(label)) / SNARK::verify(&comm, &inputs, ..)"""

    def __init__(self, proof_bytes, stage_ms=None):
        self.bytes = proof_bytes
        self.stage_ms = stage_ms

    @classmethod
    def prove(cls, inst, comm, vars_, inputs, gens, transcript_label=b"snark_example", seed=None):
        label = bytes(transcript_label)
        p, n, ms = _vp(), _sz(), (ctypes.c_double * 10)()
        if isinstance(vars_, Witness):                       # assignment already resident in HBM
            _check(lib.otti_snark_prove_resident(inst._h, comm._h, vars_._h, gens._h, label, len(label), _seed(seed), ctypes.byref(p), ctypes.byref(n), ms))
            return cls(NIZK._take(p, n), dict(zip(SNARK_STAGES, ms)))
        v, i = _scalars(vars_.assignment, "vars"), _scalars(inputs.assignment, "inputs")
        _check(lib.otti_snark_prove(inst._h, comm._h, _ptr(v), v.shape[0], _ptr(i), i.shape[0], gens._h, label, len(label), _seed(seed), 1,
                                    ctypes.byref(p), ctypes.byref(n), ms))
        return cls(NIZK._take(p, n), dict(zip(SNARK_STAGES, ms)))

    @classmethod
    def prove_sharded(cls, inst, comm, witness, gens, transcript_label=b"snark_example", seed=None):
        """This rank's part of ONE SNARK::prove spread over the GPUs of a node (collective over the ranks of ``shard_init``)."""
        label = bytes(transcript_label)
        p, n, ms = _vp(), _sz(), (ctypes.c_double * 10)()
        _check(lib.otti_snark_prove_sharded(inst._h, comm._h, witness._h, gens._h, label, len(label), _seed(seed), ctypes.byref(p), ctypes.byref(n), ms))
        return cls(NIZK._take(p, n), dict(zip(SNARK_STAGES, ms)))

    def verify(self, comm, inputs, gens, transcript_label=b"snark_example"):
        label = bytes(transcript_label)
        i = _scalars(inputs.assignment, "inputs")
        buf = np.frombuffer(self.bytes, dtype=np.uint8)
        _check(lib.otti_snark_verify(comm._h, _ptr(i), i.shape[0], gens._h, label, len(label), _ptr(buf), buf.size))

    @staticmethod
    def verify_many(comm, proofs, inputs, gens, transcript_label=b"snark_example", threads=0):
        """Many proofs of ONE computation commitment in one call (otti_snark_verify_many): ``proofs`` are SNARK objects or bytes, ``inputs`` one
        InputsAssignment for all of them or one per proof.  Returns the list of result codes — element i is what ``verify`` on proof i alone would
        report, 0 = accepted — so a rejected proof raises nothing; only the call's own refusals (bad arguments) raise.  Not a randomised batch: no
        verdict depends on another proof.  ``threads``: the library's worker threads, 0 = its default, at most 16; the call blocks until all are done."""
        label = bytes(transcript_label)
        blobs = [np.frombuffer(bytes(p.bytes if isinstance(p, SNARK) else p), dtype=np.uint8) for p in proofs]
        n = len(blobs)
        per = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs] * n
        if len(per) != n:
            raise ValueError("verify_many: one InputsAssignment for all proofs, or one per proof")
        ins = [_scalars(i.assignment, "inputs") for i in per]
        in_ptrs, in_counts = (_vp * max(1, n))(), (_sz * max(1, n))()
        pf_ptrs, pf_lens = (_vp * max(1, n))(), (_sz * max(1, n))()
        empty = np.zeros(1, dtype=np.uint8)
        for k in range(n):
            in_ptrs[k], in_counts[k] = _ptr(ins[k]), ins[k].shape[0]
            pf_ptrs[k], pf_lens[k] = (blobs[k] if blobs[k].size else empty).ctypes.data_as(_vp), blobs[k].size   # an empty proof is a malformed one, not a null pointer
        results, rejected = (_i32 * max(1, n))(), _sz(0)
        _check(lib.otti_snark_verify_many(comm._h, gens._h, label, len(label), n, in_ptrs, in_counts, pf_ptrs, pf_lens, threads, results, ctypes.byref(rejected)))
        out = [int(results[k]) for k in range(n)]
        assert rejected.value == sum(1 for r in out if r != 0)
        return out

    @staticmethod
    def verify_batch(comm, proofs, inputs, gens, transcript_label=b"snark_example", threads=0, seed=None, details=False):
        """Many proofs of ONE computation commitment as one randomised batch (otti_snark_verify_batch): the arguments and the returned list of
        codes are ``verify_many``'s — element i is what ``verify`` on proof i alone would report, except that a proof it rejects is accepted with
        probability at most 2^-120 over the library's randomness.  ``seed`` (32 bytes) repeats a run in tests; a seed the prover could know
        forfeits soundness, so leave it None.  ``details=True`` returns (codes, info dict: the otti_verify_batch_info counters)."""
        label = bytes(transcript_label)
        blobs = [np.frombuffer(bytes(p.bytes if isinstance(p, SNARK) else p), dtype=np.uint8) for p in proofs]
        n = len(blobs)
        per = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs] * n
        if len(per) != n:
            raise ValueError("verify_batch: one InputsAssignment for all proofs, or one per proof")
        ins = [_scalars(i.assignment, "inputs") for i in per]
        in_ptrs, in_counts = (_vp * max(1, n))(), (_sz * max(1, n))()
        pf_ptrs, pf_lens = (_vp * max(1, n))(), (_sz * max(1, n))()
        empty = np.zeros(1, dtype=np.uint8)
        for k in range(n):
            in_ptrs[k], in_counts[k] = _ptr(ins[k]), ins[k].shape[0]
            pf_ptrs[k], pf_lens[k] = (blobs[k] if blobs[k].size else empty).ctypes.data_as(_vp), blobs[k].size
        results, rejected, info = (_i32 * max(1, n))(), _sz(0), _VerifyBatchInfo()
        _check(lib.otti_snark_verify_batch(comm._h, gens._h, label, len(label), n, in_ptrs, in_counts, pf_ptrs, pf_lens, threads, _seed(seed), results,
                                           ctypes.byref(rejected), ctypes.byref(info)))
        out = [int(results[k]) for k in range(n)]
        assert rejected.value == sum(1 for r in out if r != 0)
        if not details:
            return out
        return out, {k: getattr(info, k) for k, _ in _VerifyBatchInfo._fields_}


def shard_init(segment_name, rank, world):
    """Join the node-local exchange of a sharded proof (collective; ``segment_name`` must be fresh and the same on every rank)."""
    _check(lib.otti_shard_init(str(segment_name).encode(), rank, world))


def shard_finalize():
    _check(lib.otti_shard_finalize())


def shard_info():
    """(rank, world, transport) of the sharded-proof exchange; transport is 'mailbox' or 'rccl' (OTTI_SHARD_TRANSPORT)"""
    r, w, t = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib.otti_shard_info(ctypes.byref(r), ctypes.byref(w), ctypes.byref(t)))
    return r.value, w.value, ("mailbox", "rccl")[t.value]


def shard_allgather(mine, world):
    """Exchange primitive: every rank's ``mine`` (bytes of equal length), concatenated in rank order."""
    mine = bytes(mine)
    out = ctypes.create_string_buffer(len(mine) * world)
    _check(lib.otti_shard_allgather(ctypes.cast(ctypes.c_char_p(mine), _vp), len(mine), ctypes.cast(out, _vp)))
    return out.raw


def shard_allreduce(scalars32):
    """Exchange primitive: element-wise sum over ranks of canonical GF(l) scalars, shape (n, 32) uint8."""
    a = np.ascontiguousarray(scalars32, dtype=np.uint8).reshape(-1, 32).copy()
    _check(lib.otti_shard_allreduce(_ptr(a), a.shape[0]))
    return a


def _seed(seed):
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("seed must be 32 bytes")
    return ctypes.cast(ctypes.create_string_buffer(seed, 32), _vp)


# ---------------------------------------------------------------------------------------------- ingest / synthetic
def _r1cs_to_py(rp):
    r = rp.contents

    def ents(p, n):
        if not n or not p:                                     # (an assignment of otti_instance_from_zkif carries counts without lists)
            return np.zeros(0, dtype=ENTRY_DTYPE)
        a = np.empty(n, dtype=ENTRY_DTYPE)                     # one memcpy (np.ctypeslib.as_array builds a ctypes array type per shape: seconds at 2^22)
        ctypes.memmove(a.ctypes.data, ctypes.cast(p, _vp), n * ENTRY_DTYPE.itemsize)
        return a

    def bytes32(p, n):
        if not n:
            return np.zeros((0, 32), dtype=np.uint8)
        a = np.empty((n, 32), dtype=np.uint8)
        ctypes.memmove(a.ctypes.data, ctypes.cast(p, _vp), n * 32)
        return a

    out = dict(num_cons=r.num_cons, num_vars=r.num_vars, num_inputs=r.num_inputs, A=ents(r.A, r.nA), B=ents(r.B, r.nB), C=ents(r.C, r.nC),
               vars=bytes32(r.vars32, r.nvars), inputs=bytes32(r.inputs32, r.ninputs))
    lib.otti_r1cs_free(rp)
    return out


def synth_r1cs(n, num_inputs=10, seed=1):
    """Synthetic satisfiable R1CS of SURVEY.md 8(d): num_cons = num_vars = n, one non-zero per row per matrix."""
    rp = ctypes.POINTER(_R1CS)()
    _check(lib.otti_synth_r1cs(n, num_inputs, seed, ctypes.byref(rp)))
    return _r1cs_to_py(rp)


def synth_r1cs_compiler_like(n, num_inputs=10, seed=1):
    """Second distribution of SURVEY.md 8(d): compiler-like R1CS (small witness values, ragged rows, heavy constant column)."""
    rp = ctypes.POINTER(_R1CS)()
    _check(lib.otti_synth_r1cs_compiler_like(n, num_inputs, seed, ctypes.byref(rp)))
    return _r1cs_to_py(rp)


def zkif_load(circuit, inputs=None, witness=None):
    rp = ctypes.POINTER(_R1CS)()
    enc = lambda s: None if s is None else os.fsencode(s)
    _check(lib.otti_zkif_load(enc(circuit), enc(inputs), enc(witness), ctypes.byref(rp)))
    return _r1cs_to_py(rp)


def zkif_write(r, circuit, inputs, witness):
    A, B, C = (np.ascontiguousarray(r[k], dtype=ENTRY_DTYPE) for k in "ABC")
    v, i = _scalars(r["vars"], "vars"), _scalars(r["inputs"], "inputs")
    s = _R1CS(r["num_cons"], r["num_vars"], r["num_inputs"], _ptr(A), _ptr(B), _ptr(C), A.size, B.size, C.size, _ptr(v), v.shape[0], _ptr(i), i.shape[0])
    _check(lib.otti_zkif_write(ctypes.byref(s), os.fsencode(circuit), os.fsencode(inputs), os.fsencode(witness)))


# ---------------------------------------------------------------------------------------------- field element helpers (tests/bench)
def fr_from_ints(xs):
    """python ints -> (n,32) uint8 Montgomery-form elements (the in-HBM layout)"""
    out = np.zeros((len(xs), 32), dtype=np.uint8)
    for k, x in enumerate(xs):
        out[k] = np.frombuffer(((x % L_ORDER) * _R % L_ORDER).to_bytes(32, "little"), dtype=np.uint8)
    return out


def fr_to_ints(a):
    a = _scalars(a, "fr")
    return [int.from_bytes(a[k].tobytes(), "little") * _RINV % L_ORDER for k in range(a.shape[0])]


KERNEL_CLASSES = ("msm_rows", "msm_small", "msm_finish", "sc_cubic", "sc_quad", "spmv", "eq", "reduce", "poly_bound", "bullet", "other",
                  "pc_round", "prod_layer", "hash_layer", "gather", "dot_many", "decode", "msm_var", "sat_check")


def stats_enable(on=True, only=None):
    _check(lib.otti_stats_enable(1 if on else 0))
    if on and only is not None:
        _check(lib.otti_stats_select(only.encode()))


def fr_mul_peak():
    """whole-chip Montgomery products in GF(l) per second (the streaming kernels' second roof), measured now"""
    v = ctypes.c_double()
    _check(lib.otti_bench_fr_mul_peak(ctypes.byref(v)))
    return v.value


def armed_launches_on():
    """whether the calling thread's next proof uses armed launches (see otti_armed_launches_on)"""
    v = _i32()
    _check(lib.otti_armed_launches_on(ctypes.byref(v)))
    return bool(v.value)


def madd_peak():
    """whole-chip mixed point additions per second (the MSM's ALU roof), measured now"""
    v = ctypes.c_double()
    _check(lib.otti_bench_madd_peak(ctypes.byref(v)))
    return v.value


def stats_read():
    """{class: (launch count, total ms)} measured with HIP events on the library's stream"""
    out = {}
    for k in KERNEL_CLASSES:
        n, ms = _u64(), ctypes.c_double()
        _check(lib.otti_stats_read(k.encode(), ctypes.byref(n), ctypes.byref(ms)))
        out[k] = (n.value, ms.value)
    return out


def lanes_pack(fr_mont):
    a = _scalars(fr_mont, "fr")
    out = np.zeros(a.shape[0] * 8, dtype=np.uint64)
    lib.otti_lanes_pack(_ptr(a), a.shape[0], _ptr(out))
    return out


def lanes_unpack(lanes):
    lanes = np.ascontiguousarray(lanes, dtype=np.uint64)
    n = lanes.size // 8
    out = np.zeros((n, 32), dtype=np.uint8)
    lib.otti_lanes_unpack(_ptr(lanes), n, _ptr(out))
    return out


class kernels:
    """Kernel-level entry points (otti_k_*): host (n,32) uint8 Montgomery arrays in, arrays out, plus kernel milliseconds."""

    @staticmethod
    def _ms():
        return ctypes.c_float(0)

    @staticmethod
    def fr_op(op, a, b):
        a, b = _scalars(a, "a"), _scalars(b, "b")
        out, ms = np.zeros_like(a), ctypes.c_float(0)
        _check(lib.otti_k_fr_op({"mul": 0, "add": 1, "sub": 2}[op], _ptr(a), _ptr(b), _ptr(out), a.shape[0], ctypes.byref(ms)))
        return out, ms.value

    FP_FORMS = ("fp8", "f9", "f10")
    FP_OPS = ("mul", "sqr", "add", "sub", "neg", "carry", "repack", "mul_sub_add", "mul_3a_2b", "mul_f_e", "mul_carried_f_g", "pow22523")
    PT_OPS = ("p9_madd", "p10_madd", "p10_add", "q10_madd", "q10_add", "chain", "encode", "decode")

    @staticmethod
    def _words(a, width, what):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError(f"{what}: expected an (n, {width}) uint8 array")
        return a

    @staticmethod
    def fp_op(form, op, a, b=None, c=None, d=None):
        """otti_k_fp_op: GF(2^255-19) in one of the device's forms (FP_FORMS) on (n, 32) uint8 little-endian words; absent operands are zero.
        Returns (packed results (n, 32) uint8, raw limbs (n, 8 | 9 | 10) uint32).  FP_OPS: a*b, a^2, a+b, a-b, -a, carry((a-b)+(c+d)),
        unpack(pack(unpack(a))), (a-b)*(c+d), (a+a+a)*(b+b), ((a+a)-b)*(c-d), carry((a+a)-b)*((c+c)+d), a^(2^252-3)."""
        a = kernels._words(a, 32, "a"); n = a.shape[0]
        b, c, d = (np.zeros_like(a) if x is None else kernels._words(x, 32, "operand") for x in (b, c, d))
        if not (b.shape == c.shape == d.shape == a.shape):
            raise ValueError("operands: one length")
        f = kernels.FP_FORMS.index(form)
        out, limbs = np.zeros_like(a), np.zeros((n, 10), dtype=np.uint32)
        _check(lib.otti_k_fp_op(f, kernels.FP_OPS.index(op), _ptr(a), _ptr(b), _ptr(c), _ptr(d), n, _ptr(out), _ptr(limbs), None))
        return out, limbs[:, :(8, 9, 10)[f]].copy()

    FR9_OPS = ("unpack", "unpack5", "unpack10", "mul", "mul_self", "add", "norm", "sub_kl2", "sub_kl4", "sub_kl8", "sub_kl16", "sub_kl128", "fold_top",
               "shl5", "pack_lt2l", "pack_lt3l", "canon", "mul9", "fold9")
    FR9_WORDS_IN = {"unpack": 1, "unpack5": 1, "unpack10": 1, "mul9": 2, "fold9": 3}      # operands that are 32-byte words; every other operand: nine limbs
    FR9_LIMBS_IN = {"mul": 2, "add": 2, "sub_kl2": 2, "sub_kl4": 2, "sub_kl8": 2, "sub_kl16": 2, "sub_kl128": 2}   # (the other limb operations: one)

    @staticmethod
    def fr9_op(op, a, b=None, c=None):
        """otti_k_fr9_op: GF(l) in nine limbs of 29 bits (fr9.h; fold9 of the round kernels), the very inline functions the hot kernels call.  An
        operand is (n, 32) uint8 (a little-endian word) or (n, 9) uint32 (raw limbs), as the operation demands (FR9_WORDS_IN; the rest take limbs);
        every operand the operation reads must be given, none that it does not.  Returns (words (n, 32) uint8, limbs (n, 9) uint32); the output an
        operation does not produce is zero.  No precondition is checked here."""
        o = kernels.FR9_OPS.index(op)
        nw = kernels.FR9_WORDS_IN.get(op, 0)
        need = nw if nw else kernels.FR9_LIMBS_IN.get(op, 1)
        given = [x for x in (a, b, c) if x is not None]
        if len(given) != need or any(x is None for x in (a, b, c)[:need]):
            raise ValueError(f"{op}: takes {need} operand(s)")
        if nw:
            given = [kernels._words(x, 32, "operand") for x in given]
        else:
            given = [np.ascontiguousarray(x, dtype=np.uint32) for x in given]
            if any(x.ndim != 2 or x.shape[1] != 9 for x in given):
                raise ValueError("operand: expected an (n, 9) uint32 array of limbs")
        n = given[0].shape[0]
        if any(x.shape != given[0].shape for x in given):
            raise ValueError("operands: one length")
        given += [given[0]] * (3 - need)                              # never read: the entry only wants no null pointer
        out, limbs = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 9), dtype=np.uint32)
        _check(lib.otti_k_fr9_op(o, _ptr(given[0]), _ptr(given[1]), _ptr(given[2]), n, _ptr(out), _ptr(limbs), None))
        return out, limbs

    @staticmethod
    def pt_op(op, P, Q=None, neg=False, k=1):
        """otti_k_pt_op (PT_OPS).  The formulas: P (n, 128) points, Q (n, 96) Niels entries (p9_madd, p10_madd, q10_madd, chain: k additions of the
        same entry) or (n, 128) points (p10_add, q10_add); returns (packed points (n, 128) uint8, raw limbs (n, 4, 9 | 10) uint32).
        encode: k_encode_points on P, on P[i] + Q[i] with Q; returns (n, 32) encodings.  decode: k_decode_niels on P (n, 32) encodings; returns
        (Niels entries (n, 96), the number refused)."""
        o = kernels.PT_OPS.index(op)
        if op == "decode":
            P = kernels._words(P, 32, "P"); n = P.shape[0]
            out, bad = np.zeros((n, 96), dtype=np.uint8), _u32(0)
            _check(lib.otti_k_pt_op(o, _ptr(P), None, 0, 0, n, _ptr(out), None, ctypes.byref(bad), None))
            return out, bad.value
        P = kernels._words(P, 128, "P"); n = P.shape[0]
        if op == "encode":
            Q = None if Q is None else kernels._words(Q, 128, "Q")
            if Q is not None and Q.shape != P.shape:
                raise ValueError("P and Q: one length")
            out = np.zeros((n, 32), dtype=np.uint8)
            _check(lib.otti_k_pt_op(o, _ptr(P), _ptr(Q), 0, 0, n, _ptr(out), None, None, None))
            return out
        Q = kernels._words(Q, 128 if op in ("p10_add", "q10_add") else 96, "Q")
        if Q.shape[0] != n:
            raise ValueError("P and Q: one length")
        out, limbs = np.zeros((n, 128), dtype=np.uint8), np.zeros((n, 4, 10), dtype=np.uint32)
        _check(lib.otti_k_pt_op(o, _ptr(P), _ptr(Q), 1 if neg else 0, int(k), n, _ptr(out), _ptr(limbs), None, None))
        return out, limbs[:, :, :(9 if op in ("p9_madd", "chain") else 10)].copy()

    @staticmethod
    def addr_timestamps(addr3, M):
        """addr3: (3, N) uint32 addresses below M.  Returns (read_ts (3, N) uint32, audit (M,) uint32, kernel ms)"""
        a = np.ascontiguousarray(addr3, dtype=np.uint32)
        if a.ndim != 2 or a.shape[0] != 3:
            raise ValueError("addr3: expected a (3, N) uint32 array")
        ts, audit, ms = np.zeros_like(a), np.zeros(int(M), dtype=np.uint32), ctypes.c_float(0)
        _check(lib.otti_k_addr_timestamps(_ptr(a), a.shape[1], int(M), _ptr(ts), _ptr(audit), ctypes.byref(ms)))
        return ts, audit, ms.value

    @staticmethod
    def decomm_entries(row, col, val, N, pad_to=None, pad_col=0):
        """otti_k_decomm_entries: one matrix of the SNARK decommitment from an entry list (row, col: uint32; val: (n, 32) Montgomery).  pad_to: the
        explicit padding's end (None: n, no padding).  Returns (row_u32 (N,), col_u32 (N,), row_fr, col_fr, val_fr ((N, 32) each), kernel ms)"""
        row, col = np.ascontiguousarray(row, dtype=np.uint32), np.ascontiguousarray(col, dtype=np.uint32)
        val = _scalars(val, "val") if len(val) else np.zeros((0, 32), dtype=np.uint8)
        n, N = row.size, int(N)
        if col.size != n or val.shape[0] != n:
            raise ValueError("row, col and val: one length")
        ru, cu = np.zeros(max(N, 0), dtype=np.uint32), np.zeros(max(N, 0), dtype=np.uint32)
        fr = [np.zeros((max(N, 0), 32), dtype=np.uint8) for _ in range(3)]; ms = ctypes.c_float(0)
        _check(lib.otti_k_decomm_entries(_ptr(row) if n else None, _ptr(col) if n else None, _ptr(val) if n else None, n, N, n if pad_to is None else int(pad_to), int(pad_col),
                                         _ptr(ru), _ptr(cu), _ptr(fr[0]), _ptr(fr[1]), _ptr(fr[2]), ctypes.byref(ms)))
        return ru, cu, fr[0], fr[1], fr[2], ms.value

    @staticmethod
    def shard_filter(row, col, val, world, rank, by_col=False):
        """otti_k_shard_filter: rank's share of an entry list, in order, the row (by_col: column) divided by world.  Returns (row, col, val, kernel ms)"""
        row, col = np.ascontiguousarray(row, dtype=np.uint32), np.ascontiguousarray(col, dtype=np.uint32)
        val = _scalars(val, "val") if len(val) else np.zeros((0, 32), dtype=np.uint8)
        n = row.size
        if col.size != n or val.shape[0] != n:
            raise ValueError("row, col and val: one length")
        orow, ocol, oval = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros((n, 32), dtype=np.uint8)
        cnt, ms = _sz(), ctypes.c_float(0)
        p = (lambda a: _ptr(a) if n else None)
        _check(lib.otti_k_shard_filter(p(row), p(col), p(val), n, int(world), int(rank), 1 if by_col else 0, p(orow), p(ocol), p(oval), ctypes.byref(cnt), ctypes.byref(ms)))
        k = cnt.value
        return orow[:k].copy(), ocol[:k].copy(), oval[:k].copy(), ms.value

    @staticmethod
    def from_canonical(a):
        a = _scalars(a, "a"); out = np.zeros_like(a)
        _check(lib.otti_k_fr_from_canonical(_ptr(a), _ptr(out), a.shape[0])); return out

    @staticmethod
    def to_canonical(a):
        a = _scalars(a, "a"); out = np.zeros_like(a)
        _check(lib.otti_k_fr_to_canonical(_ptr(a), _ptr(out), a.shape[0])); return out

    @staticmethod
    def multiply_vec(inst, z):
        z = _scalars(z, "z"); nc, nv, _ = inst.dims
        assert z.shape[0] == 2 * nv
        o = [np.zeros((nc, 32), dtype=np.uint8) for _ in range(3)]; ms = ctypes.c_float(0)
        _check(lib.otti_k_multiply_vec(inst._h, _ptr(z), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), ctypes.byref(ms)))
        return o[0], o[1], o[2], ms.value

    @staticmethod
    def multiply_vec_many(inst, zs):
        """otti_k_multiply_vec_many: Az, Bz, Cz of the K vectors ``zs`` through the many-vector kernels, a tile of four per walk over the matrices.
        Returns ((K, N, 32) Az, Bz, Cz, kernel ms)."""
        zs = [np.ascontiguousarray(_scalars(z, "z")) for z in zs]; nc, nv, _ = inst.dims; K = len(zs)
        assert K and all(z.shape[0] == 2 * nv for z in zs)
        ptrs = (_vp * K)(*[_ptr(z) for z in zs])
        o = [np.zeros((K, nc, 32), dtype=np.uint8) for _ in range(3)]; ms = ctypes.c_float(0)
        _check(lib.otti_k_multiply_vec_many(inst._h, ptrs, K, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), ctypes.byref(ms)))
        return o[0], o[1], o[2], ms.value

    @staticmethod
    def prove_front(inst, gens, zs, small_flags):
        """otti_k_prove_front: prove_many's front half alone on the K staged vectors ``zs``.  Returns ((K, L, 32) compressed unblinded row sums,
        (K, N, 32) Az, Bz, Cz, info dict, ms)."""
        zs = [np.ascontiguousarray(_scalars(z, "z")) for z in zs]; nc, nv, _ = inst.dims; K = len(zs)
        assert K and all(z.shape[0] == 2 * nv for z in zs) and len(small_flags) == K
        ell = nv.bit_length() - 1; L = 1 << (ell // 2)
        ptrs = (_vp * K)(*[_ptr(z) for z in zs])
        flags = np.ascontiguousarray([1 if f else 0 for f in small_flags], dtype=np.int32)
        rows = np.zeros((K, L, 32), dtype=np.uint8)
        o = [np.zeros((K, nc, 32), dtype=np.uint8) for _ in range(3)]; ms = ctypes.c_float(0); info = _ProveManyInfo()
        _check(lib.otti_k_prove_front(inst._h, gens._h, ptrs, _ptr(flags), K, _ptr(rows), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), ctypes.byref(info), ctypes.byref(ms)))
        return rows, o[0], o[1], o[2], info.as_dict(), ms.value

    @staticmethod
    def products_patch(inst, z_new, Az, Bz, Cz, bits, n_unsat, cols=None, first=0, count=0):
        """otti_k_products_patch: the kept-products patch on host state.  Az, Bz, Cz ((N, 32) uint8 Montgomery words) and bits (uint64 words) are
        copied, patched for ``z_new`` and the changed columns (``cols``: ascending uint64 array; None: the range first, count) and returned:
        (Az, Bz, Cz, bits, n_unsat, touched rows ascending (uint32), took_full_pass, kernel_ms)"""
        z = _scalars(z_new, "z"); nc, nv, _ = inst.dims
        assert z.shape[0] == 2 * nv
        o = [np.ascontiguousarray(_scalars(x, "products")).copy() for x in (Az, Bz, Cz)]
        b = np.ascontiguousarray(bits, dtype=np.uint64).copy()
        assert all(x.shape[0] == nc for x in o) and b.size == (nc + 63) // 64
        if cols is not None:
            cols = np.ascontiguousarray(cols, dtype=np.uint64)
        rows = np.zeros(nc, dtype=np.uint32)
        u, nt, full, ms = _u64(n_unsat), _u64(), _i32(), ctypes.c_float(0)
        _check(lib.otti_k_products_patch(inst._h, _ptr(z), _ptr(cols) if cols is not None else None, cols.size if cols is not None else 0, first, count,
                                         _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(b), ctypes.byref(u), _ptr(rows), nc, ctypes.byref(nt), ctypes.byref(full), ctypes.byref(ms)))
        return o[0], o[1], o[2], b, u.value, rows[:nt.value].copy(), bool(full.value), ms.value

    @staticmethod
    def eval_table_sparse(inst, eq_rx, rABC):
        eq_rx, rABC = _scalars(eq_rx, "eq_rx"), _scalars(rABC, "rABC"); nc, nv, _ = inst.dims
        assert eq_rx.shape[0] == nc and rABC.shape[0] == 3
        out = np.zeros((2 * nv, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_eval_table_sparse(inst._h, _ptr(eq_rx), _ptr(rABC), _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def instance_evaluate(inst, rx, ry):
        """otti_k_instance_evaluate: A, B, C at K points in one batched pass.  rx: (K, log2 num_cons, 32), ry: (K, log2(2 num_vars), 32) Montgomery
        words (or the same flattened to (K * ell, 32)); returns ((K, 3, 32) Montgomery words, kernel_ms)"""
        nc, nv, _ = inst.dims
        nrx, nry = nc.bit_length() - 1, (2 * nv).bit_length() - 1
        rx = np.ascontiguousarray(rx, dtype=np.uint8).reshape(-1, 32); ry = np.ascontiguousarray(ry, dtype=np.uint8).reshape(-1, 32)
        k = rx.shape[0] // nrx if nrx else ry.shape[0] // nry
        assert rx.shape[0] == k * nrx and ry.shape[0] == k * nry
        out = np.zeros((k, 3, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_instance_evaluate(inst._h, _ptr(rx), _ptr(ry), k, _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def eq_evals(r):
        r = _scalars(r, "r"); ell = r.shape[0]
        out = np.zeros((1 << ell, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_eq_evals(_ptr(r), ell, _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def fold_top(Z, r):
        Z, r = _scalars(Z, "Z"), _scalars(r, "r"); out = np.zeros((Z.shape[0] // 2, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_fold_top(_ptr(Z), Z.shape[0], _ptr(r), _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def fold_bot(Z, r):
        Z, r = _scalars(Z, "Z"), _scalars(r, "r"); out = np.zeros((Z.shape[0] // 2, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_fold_bot(_ptr(Z), Z.shape[0], _ptr(r), _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def sc_cubic_round(A, B, C, D):
        A, B, C, D = (_scalars(x, "t") for x in (A, B, C, D)); e = np.zeros((3, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_sc_cubic_round(_ptr(A), _ptr(B), _ptr(C), _ptr(D), A.shape[0], _ptr(e), ctypes.byref(ms)))
        return e, ms.value

    @staticmethod
    def sc_cubic_fold_round(A, B, C, D, r):
        A, B, C, D, r = (_scalars(x, "t") for x in (A, B, C, D, r)); n = A.shape[0]
        out = np.zeros((4, n // 2, 32), dtype=np.uint8); e = np.zeros((3, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_sc_cubic_fold_round(_ptr(A), _ptr(B), _ptr(C), _ptr(D), n, _ptr(r), _ptr(out), _ptr(e), ctypes.byref(ms)))
        return out, e, ms.value

    @staticmethod
    def sc_quad_round(A, B):
        A, B = _scalars(A, "A"), _scalars(B, "B"); e = np.zeros((2, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_sc_quad_round(_ptr(A), _ptr(B), A.shape[0], _ptr(e), ctypes.byref(ms)))
        return e, ms.value

    @staticmethod
    def sc_quad_fold_round(A, B, r):
        A, B, r = (_scalars(x, "t") for x in (A, B, r)); n = A.shape[0]
        out = np.zeros((2, n // 2, 32), dtype=np.uint8); e = np.zeros((2, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_sc_quad_fold_round(_ptr(A), _ptr(B), n, _ptr(r), _ptr(out), _ptr(e), ctypes.byref(ms)))
        return out, e, ms.value

    SC_KINDS = ("cubic3_eval", "cubic3_fold", "quad_eval", "quad_fold", "cubic4_eval", "cubic4_fold")     # sc_plan.h ScKind

    @staticmethod
    def sc_plan(kind, n, armed=False):
        """otti_k_sc_plan: (workgroups, the most items a thread walks) of a round launch of ``kind`` (SC_KINDS) over tables of length n, under the
        capacities now in force (the device's own, or those of an enclosing sc_caps)"""
        wg, per = ctypes.c_uint32(0), _u64(0)
        _check(lib.otti_k_sc_plan(kernels.SC_KINDS.index(kind), n, 1 if armed else 0, ctypes.byref(wg), ctypes.byref(per)))
        return wg.value, per.value

    @staticmethod
    @contextlib.contextmanager
    def sc_caps(num_cu, resident):
        """otti_k_sc_caps_override for the length of a ``with`` block: the round launches inside take their grids from ``num_cu`` CUs and ``resident``
        workgroups at once (one number for all six kernels, or six by SC_KINDS) in the device's place; the device's own return on the way out"""
        res = [int(resident)] * 6 if np.isscalar(resident) else [int(x) for x in resident]
        if len(res) != 6:
            raise ValueError("resident: one number or six")
        caps = (ctypes.c_uint32 * 7)(int(num_cu), *res)
        _check(lib.otti_k_sc_caps_override(caps))
        try:
            yield
        finally:
            _check(lib.otti_k_sc_caps_override(None))

    @staticmethod
    def sc_caps_restore():
        """the device's own capacities again, whatever override stands"""
        _check(lib.otti_k_sc_caps_override(None))

    @staticmethod
    def armed_selftest(A, B, r, hold_us=200):
        """plain / armed + released / armed + aborted runs of the quadratic fold round; returns the plain run's (folded tables, sums)"""
        A, B, r = (_scalars(x, "t") for x in (A, B, r)); n = A.shape[0]
        out = np.zeros((2, n // 2, 32), dtype=np.uint8); e = np.zeros((2, 32), dtype=np.uint8)
        _check(lib.otti_k_armed_selftest(_ptr(A), _ptr(B), n, _ptr(r), hold_us, _ptr(out), _ptr(e)))
        return out, e

    @staticmethod
    def row_sum(compressed, scalars_mont):
        """the verifier's variable-base sum on the device: compress(sum_i s[i] * decompress(C[i]))"""
        C = np.ascontiguousarray(compressed, dtype=np.uint8).reshape(-1, 32); s = _scalars(scalars_mont, "s")
        assert C.shape[0] == s.shape[0]
        out = np.zeros(32, dtype=np.uint8)
        _check(lib.otti_k_row_sum(_ptr(C), C.shape[0], _ptr(s), _ptr(out)))
        return out

    @staticmethod
    def row_sum_many(sets, jobs):
        """several such sums in one pass: ``sets`` = arrays of compressed points, ``jobs`` = [(set index, Montgomery scalars)]; returns
        (sums (njobs, 32) uint8, codes [int]) — a job whose set has an undecodable point carries OTTI_ERR_VERIFY_DECOMPRESS and zeros"""
        cs = [np.ascontiguousarray(c, dtype=np.uint8).reshape(-1, 32) for c in sets]
        off = np.zeros(len(cs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([c.shape[0] for c in cs])
        comp = np.ascontiguousarray(np.concatenate(cs) if cs else np.zeros((1, 32), dtype=np.uint8))
        js = np.ascontiguousarray([k for k, _ in jobs], dtype=np.uint32)
        ss = [_scalars(s, "s") for _, s in jobs]
        for (k, _), s in zip(jobs, ss):
            assert not 0 <= k < len(cs) or s.shape[0] == cs[k].shape[0]
        sc = np.ascontiguousarray(np.concatenate(ss) if ss else np.zeros((1, 32), dtype=np.uint8))
        out = np.zeros((max(1, len(jobs)), 32), dtype=np.uint8); codes = (_i32 * max(1, len(jobs)))()
        _check(lib.otti_k_row_sum_many(len(cs), _ptr(comp), _ptr(off), len(jobs), _ptr(js), _ptr(sc), _ptr(out), codes))
        return out[:len(jobs)], [int(codes[j]) for j in range(len(jobs))]

    @staticmethod
    def batch_sum(sets, jobs):
        """the batch verifier's device pass alone (otti_k_batch_sum): ``sets`` = arrays of compressed points, lying one behind the other; with two
        sets or more the last one is decoded ahead and resident, as the generators are.  ``jobs`` = [(first set, number of sets, Montgomery
        scalars for those sets' points)].  Returns (sums (njobs, 32) uint8, codes [int], device-event ms of the launches)"""
        cs = [np.ascontiguousarray(c, dtype=np.uint8).reshape(-1, 32) for c in sets]
        off = np.zeros(len(cs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([c.shape[0] for c in cs])
        comp = np.ascontiguousarray(np.concatenate(cs) if cs else np.zeros((1, 32), dtype=np.uint8))
        first = np.ascontiguousarray([f for f, _, _ in jobs], dtype=np.uint32); count = np.ascontiguousarray([c for _, c, _ in jobs], dtype=np.uint32)
        ss = [_scalars(s, "s") for _, _, s in jobs]
        for (f, c, _), s in zip(jobs, ss):
            assert not (c >= 1 and 0 <= f and f + c <= len(cs)) or s.shape[0] == int(off[f + c] - off[f])
        sc = np.ascontiguousarray(np.concatenate(ss) if ss else np.zeros((1, 32), dtype=np.uint8))
        out = np.zeros((max(1, len(jobs)), 32), dtype=np.uint8); codes = (_i32 * max(1, len(jobs)))(); ms = ctypes.c_float(0)
        _check(lib.otti_k_batch_sum(len(cs), _ptr(comp), _ptr(off), len(jobs), _ptr(first), _ptr(count), _ptr(sc), _ptr(out), codes, ctypes.byref(ms)))
        return out[:len(jobs)], [int(codes[j]) for j in range(len(jobs))], float(ms.value)

    @staticmethod
    def gen_runs(jobs):
        """the expansion of product-form generator runs alone (otti_k_gen_runs): ``jobs`` = [(n, base, runs)] with ``base`` n Montgomery scalars
        or None and ``runs`` = [(coefficient, factors)], Montgomery, a run of lg factors covering slots [0, 2^lg) of its job.  Returns (one
        (n, 32) Montgomery array per job: base[i] + sum of c * prod of the factors at the set bits of i, device-event ms)"""
        ns = np.ascontiguousarray([n for n, _, _ in jobs], dtype=np.uint64)
        has = np.ascontiguousarray([b is not None for _, b, _ in jobs], dtype=np.uint8)
        bs = [_scalars(b, "base") for _, b, _ in jobs if b is not None]
        for n, b, _ in jobs:
            assert b is None or _scalars(b, "base").shape[0] == n
        base = np.ascontiguousarray(np.concatenate(bs)) if bs else None
        rj, rl, rc, rf = [], [], [], []
        for j, (_, _, runs) in enumerate(jobs):
            for c, f in runs:
                f = _scalars(f, "factors") if len(f) else np.zeros((0, 32), dtype=np.uint8)
                rj.append(j); rl.append(f.shape[0]); rc.append(_scalars(c, "c").reshape(1, 32)); rf.append(f)
        run_job = np.ascontiguousarray(rj, dtype=np.uint32); run_lg = np.ascontiguousarray(rl, dtype=np.uint32)
        cs = np.ascontiguousarray(np.concatenate(rc)) if rc else None
        fs = np.ascontiguousarray(np.concatenate(rf)) if rf else None
        out = np.zeros((max(1, int(ns.sum())), 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_gen_runs(len(jobs), _ptr(ns), _ptr(has), _ptr(base), len(rj), _ptr(run_job), _ptr(run_lg), _ptr(cs), _ptr(fs), _ptr(out), ctypes.byref(ms)))
        cut = np.cumsum(ns).astype(np.int64)[:-1]
        return np.split(out[:int(ns.sum())], cut), float(ms.value)

    @staticmethod
    def msm_scatter_rows(gens, L, idx, s):
        """the kernel that patches kept rows, onto L identity points: row i = compress(sum of s[k] * P[idx[k] - i R] over its indices)"""
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        s = _scalars(s, "s")
        out = np.zeros((L, 32), dtype=np.uint8)
        ms = kernels._ms()
        _check(lib.otti_k_msm_scatter_rows(gens._h, L, _ptr(idx), _ptr(s), idx.size, _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def witness_diff(old, src, fmt, stride_bytes=0):
        """otti_witness_assign's two passes on staged vectors: ``old`` (n, 32) Montgomery words, ``src`` the raw bytes of n elements in ``fmt``,
        ``stride_bytes`` apart (0: packed).  Returns (the new vector, the ascending changed indices, their deltas new - old, elements per chunk)."""
        old = _scalars(old, "old")
        n = old.shape[0]
        raw = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        eb = 8 if fmt in (WIT_I64, WIT_U64) else 32
        if n and raw.size < (n - 1) * (stride_bytes or eb) + eb:
            raise ValueError("src is shorter than n elements at this stride")
        new, idx, delta = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint64), np.zeros((n, 32), dtype=np.uint8)
        k, chunk = _u64(), ctypes.c_uint32()
        _check(lib.otti_k_witness_diff(_ptr(old), n, _ptr(raw), fmt, stride_bytes, _ptr(new), _ptr(idx), _ptr(delta), ctypes.byref(k), ctypes.byref(chunk), None))
        return new, idx[:k.value].copy(), delta[:k.value].copy(), chunk.value

    @staticmethod
    def msm_rows(gens, Z, L, R, blinds):
        Z, blinds = _scalars(Z, "Z"), _scalars(blinds, "blinds")
        assert Z.shape[0] == L * R and blinds.shape[0] == L
        out = np.zeros((L, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_msm_rows(gens._h, _ptr(Z), L, R, _ptr(blinds), _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    MSM_MODES = ("compressed", "raw", "keep")
    MSM_KERNELS = ("bulk", "bulk_sparse", "small")
    MSM_ROUTES = ("mail", "flag", "keep", "raw", "device_encode", "host_encode")

    @staticmethod
    def msm_job(gens, rows, dense=None, extra_s=None, extra_base=(), mode="compressed", sparse=-1, force_bulk=False, bulk_workgroups=0):
        """a general fixed-base MSM job through the prover's launcher: ``dense`` (rows * n_dense, 32) Montgomery scalars, dense term j on generator
        j; ``extra_s`` (rows * n_extra, 32) on the bases ``extra_base``.  Returns (rows compressed points — in every mode —, the plan the launch
        took: dict(kernel, chunk, nchunks, fuse, route), kernel ms)."""
        base = np.ascontiguousarray(extra_base, dtype=np.uint32).reshape(-1)
        n_extra = base.size
        d = _scalars(dense, "dense") if dense is not None else np.zeros((0, 32), dtype=np.uint8)
        e = _scalars(extra_s, "extra_s") if extra_s is not None else np.zeros((0, 32), dtype=np.uint8)
        if rows < 1 or d.shape[0] % rows or e.shape[0] != rows * n_extra:
            raise ValueError("msm_job: dense is rows * n_dense scalars, extra_s rows * len(extra_base)")
        out = np.zeros((rows, 32), dtype=np.uint8); plan = np.zeros(5, dtype=np.uint32); ms = ctypes.c_float(0)
        _check(lib.otti_k_msm_job(gens._h, rows, d.shape[0] // rows, _ptr(d), n_extra, _ptr(e), _ptr(base), kernels.MSM_MODES.index(mode), int(sparse),
                                  1 if force_bulk else 0, bulk_workgroups, _ptr(out), _ptr(plan), ctypes.byref(ms)))
        return out, dict(kernel=kernels.MSM_KERNELS[plan[0]], chunk=int(plan[1]), nchunks=int(plan[2]), fuse=int(plan[3]), route=kernels.MSM_ROUTES[plan[4]]), ms.value

    # ---- the kernels the prover itself launches (phase one without the eq table, evaluation proof, bullet reduction)
    @staticmethod
    def eq_pyramid(r):
        r = _scalars(r, "r"); n = r.shape[0]
        out = np.zeros(((2 << n) - 1, 32), dtype=np.uint8)
        _check(lib.otti_k_eq_pyramid(_ptr(r), n, _ptr(out)))
        return out

    @staticmethod
    def sc_cubic3_round(B, C, D, tau):
        B, C, D, tau = (_scalars(x, "t") for x in (B, C, D, tau)); e = np.zeros((3, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        assert (1 << (tau.shape[0] + 1)) == B.shape[0]
        _check(lib.otti_k_sc_cubic3_round(_ptr(B), _ptr(C), _ptr(D), B.shape[0], _ptr(tau), _ptr(e), ctypes.byref(ms)))
        return e, ms.value

    @staticmethod
    def sc_cubic3_fold_round(B, C, D, r, tau):
        B, C, D, r, tau = (_scalars(x, "t") for x in (B, C, D, r, tau)); n = B.shape[0]
        assert (1 << (tau.shape[0] + 2)) == n
        out = np.zeros((3, n // 2, 32), dtype=np.uint8); e = np.zeros((3, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_sc_cubic3_fold_round(_ptr(B), _ptr(C), _ptr(D), n, _ptr(r), _ptr(tau), _ptr(out), _ptr(e), ctypes.byref(ms)))
        return out, e, ms.value

    @staticmethod
    def poly_bound(Z, L, R, Lv):
        Z, Lv = _scalars(Z, "Z"), _scalars(Lv, "Lv"); assert Z.shape[0] == L * R and Lv.shape[0] == L
        out = np.zeros((R, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_poly_bound(_ptr(Z), L, R, _ptr(Lv), _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def bullet_round(gens, n_cur, a, b, s, blinds2, u=None, uinv=None):
        """one bullet-reduction round on the original generators; (u, uinv) given => the previous challenge is applied first"""
        a, b, s, blinds2 = (_scalars(x, "t") for x in (a, b, s, blinds2)); R = s.shape[0]
        fold = u is not None
        uu = _scalars(u, "u") if fold else None; ui = _scalars(uinv, "uinv") if fold else None
        ao, bo, so = (np.zeros((k, 32), dtype=np.uint8) for k in (n_cur, n_cur, R)); LR = np.zeros((2, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_bullet_round(gens._h, n_cur, 1 if fold else 0, _ptr(uu), _ptr(ui), _ptr(a), _ptr(b), _ptr(s), _ptr(blinds2), _ptr(ao), _ptr(bo), _ptr(so),
                                       _ptr(LR), ctypes.byref(ms)))
        return LR, ao, bo, so, ms.value

    @staticmethod
    def bullet_last_fold(a2, b2, s, u, uinv):
        a2, b2, s, u, uinv = (_scalars(x, "t").copy() for x in (a2, b2, s, u, uinv))
        _check(lib.otti_k_bullet_last_fold(s.shape[0], _ptr(u), _ptr(uinv), _ptr(a2), _ptr(b2), _ptr(s)))
        return a2[:1], b2[:1], s

    # ---- SNARK mode's kernels (k_snark.hip).  A batch is a list with one (n, 32) table per instance; C[y] is None for a product-circuit instance
    @staticmethod
    def _stack(tables, what, n=None):
        """tables of one length as one contiguous array (the C ABI's layout); unequal lengths are the library's bad-argument error"""
        ts = [_scalars(t, what) for t in tables]
        if n is None:
            n = ts[0].shape[0] if ts else 0
        if any(t.shape[0] != n for t in ts):
            raise SpartanError(-21, f"{what}: tables of unequal length")
        return (np.concatenate(ts) if len(ts) > 1 else ts[0] if ts else np.zeros((0, 32), dtype=np.uint8)), n

    @staticmethod
    def _batch(A, B, C):
        if not (len(A) == len(B) == len(C)):
            raise SpartanError(-21, "a batch needs one A, B and C entry per instance")
        a, n = kernels._stack(A, "A"); b, _ = kernels._stack(B, "B", n)
        has_c = np.array([0 if t is None else 1 for t in C], dtype=np.uint8)
        c, _ = kernels._stack([t for t in C if t is not None], "C", n)
        return a, b, c, has_c, len(A), n

    @staticmethod
    def _unbatch(out, has_c, ninst, n_out):
        """(3 * ninst * n_out) elements laid out [(3 y + t) * n_out ..) -> per instance [A, B, C or None]"""
        o = out.reshape(ninst, 3, n_out, 32)
        return [[o[y, 0], o[y, 1], o[y, 2] if has_c[y] else None] for y in range(ninst)]

    @staticmethod
    def pc_round(A, B, C, tau, r=None, G=1, rk=0):
        """one round of the batched sum-check (dev_pc_eval, or dev_pc_fold_eval when r is given).  Returns (sums (ninst, 3, 32), folded, ms);
        folded = (A, B, C) lists of the tables folded by r (None entries where C has none), or None without r"""
        a, b, c, has_c, ninst, n = kernels._batch(A, B, C)
        tau = _scalars(tau, "tau"); rr = None if r is None else _scalars(r, "r")
        items = (n // (2 if rr is None else 4)) * G
        if ninst and items >= 1 and tau.shape[0] != items.bit_length() - 1:
            raise SpartanError(-21, "tau: one variable per bit of the eq table's index")
        h = n // 2; nc = int(has_c.sum())
        out = np.zeros(((2 * ninst + nc) * h, 32), dtype=np.uint8) if rr is not None else None
        e = np.zeros((max(ninst, 1), 3, 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_pc_round(_ptr(a), _ptr(b), _ptr(c), _ptr(has_c), ninst, n, _ptr(tau), _ptr(rr), G, rk, _ptr(out), _ptr(e), ctypes.byref(ms)))
        folded = None
        if rr is not None:
            o = out.reshape(2 * ninst + nc, h, 32); k = iter(range(2 * ninst, 2 * ninst + nc))
            folded = ([o[y] for y in range(ninst)], [o[ninst + y] for y in range(ninst)], [o[next(k)] if has_c[y] else None for y in range(ninst)])
        return e, folded, ms.value

    @staticmethod
    def pc_plan(ninst, items):
        """otti_k_pc_plan: (workgroups per instance, the most items a thread walks) of a launch of pc_round, dot_many or sum3 over ``ninst`` instances
        of ``items`` items (pc_round: n / 2, with a fold n / 4; the others: n), under the block cap now in force (the device's own 2048, or that of
        an enclosing pc_grid_cap)"""
        wg, per = ctypes.c_uint32(0), _u64(0)
        _check(lib.otti_k_pc_plan(ninst, items, ctypes.byref(wg), ctypes.byref(per)))
        return wg.value, per.value

    @staticmethod
    @contextlib.contextmanager
    def pc_grid_cap(max_blocks):
        """otti_k_pc_grid_cap_override for the length of a ``with`` block: the launches inside share ``max_blocks`` workgroups among their instances
        in the place of the device's own 2048 (``ninst`` of them: one workgroup per instance); the device's own return on the way out"""
        _check(lib.otti_k_pc_grid_cap_override(ctypes.byref(ctypes.c_uint32(int(max_blocks)))))
        try:
            yield
        finally:
            _check(lib.otti_k_pc_grid_cap_override(None))

    @staticmethod
    def pc_grid_cap_restore():
        """the device's own block cap again, whatever override stands"""
        _check(lib.otti_k_pc_grid_cap_override(None))

    @staticmethod
    def pc_export(A, B, C, fold_r=None):
        """dev_pc_export: per instance [A, B, C or None], folded by fold_r first when given"""
        a, b, c, has_c, ninst, n = kernels._batch(A, B, C)
        rr = None if fold_r is None else _scalars(fold_r, "fold_r")
        n_out = n if rr is None else n // 2
        out = np.zeros((3 * ninst * n_out, 32), dtype=np.uint8)
        _check(lib.otti_k_pc_export(_ptr(a), _ptr(b), _ptr(c), _ptr(has_c), ninst, n, _ptr(rr), _ptr(out)))
        return kernels._unbatch(out, has_c, ninst, n_out)

    @staticmethod
    def pc_tail(A, B, C, W, t_out, tau, rs, fold_r=None, top=False):
        """dev_pc_tail with the host's side of its rounds.  Returns (sums (rounds, ninst, 3, 32), tables per instance [A, B, C or None] of t_out elements)"""
        a, b, c, has_c, ninst, n = kernels._batch(A, B, C)
        rr = None if fold_r is None else _scalars(fold_r, "fold_r")
        len0 = n if rr is None else n // 2
        tau, rs = _scalars(tau, "tau"), _scalars(rs, "rs")
        W, t_out = int(W), int(t_out)
        ok = ninst and W > 0 and t_out > 0 and len0 > t_out and len0 & (len0 - 1) == 0 and t_out & (t_out - 1) == 0
        rounds = (len0.bit_length() - t_out.bit_length()) if ok else 1
        if ok and (tau.shape[0] != len0.bit_length() - 1 or rs.shape[0] != rounds):
            raise SpartanError(-21, "tau: log2(len0) variables; rs: one challenge per round")
        sums = np.zeros((rounds, max(ninst, 1), 3, 32), dtype=np.uint8); out = np.zeros((3 * max(ninst, 1) * t_out, 32), dtype=np.uint8)
        _check(lib.otti_k_pc_tail(_ptr(a), _ptr(b), _ptr(c), _ptr(has_c), ninst, len0, W, t_out, _ptr(tau), _ptr(rs), _ptr(rr), 1 if top else 0, _ptr(sums), _ptr(out)))
        return sums, kernels._unbatch(out, has_c, ninst, t_out)

    @staticmethod
    def prod_layer(in_left, in_right):
        """dev_prod_layer: per circuit (out_left, out_right), each half as long as the inputs"""
        if len(in_left) != len(in_right):
            raise SpartanError(-21, "one left and one right input per circuit")
        l, n = kernels._stack(in_left, "in_left"); r, _ = kernels._stack(in_right, "in_right", n)
        if n % 2:
            raise SpartanError(-21, "a layer's inputs have an even number of elements")
        k, q = len(in_left), n // 2
        ol, orr = (np.zeros((max(k * q, 1), 32), dtype=np.uint8) for _ in range(2)); ms = ctypes.c_float(0)
        _check(lib.otti_k_prod_layer(_ptr(l), _ptr(r), k, q, _ptr(ol), _ptr(orr), ctypes.byref(ms)))
        return [(ol[y * q:(y + 1) * q], orr[y * q:(y + 1) * q]) for y in range(k)], ms.value

    @staticmethod
    def hash_mem(eval_table, audit_ts, r, gamma, G=1, rk=0):
        """dev_hash_mem: (init, audit) hashes of rank rk's residue class (M / G elements each)"""
        ev, n = kernels._stack([eval_table], "eval_table"); au, _ = kernels._stack([audit_ts], "audit_ts", n)
        r, gamma = _scalars(r, "r"), _scalars(gamma, "gamma")
        o = [np.zeros((max(n // G, 1), 32), dtype=np.uint8) for _ in range(2)]; ms = ctypes.c_float(0)
        _check(lib.otti_k_hash_mem(_ptr(ev), _ptr(au), n, _ptr(r), _ptr(gamma), G, rk, _ptr(o[0]), _ptr(o[1]), ctypes.byref(ms)))
        return o[0], o[1], ms.value

    @staticmethod
    def hash_ops(addr, deref, read_ts, r, gamma, G=1, rk=0):
        """dev_hash_ops: (read, write) hashes of rank rk's residue class (N / G elements each)"""
        ad, n = kernels._stack([addr], "addr"); de, _ = kernels._stack([deref], "deref", n); ts, _ = kernels._stack([read_ts], "read_ts", n)
        r, gamma = _scalars(r, "r"), _scalars(gamma, "gamma")
        o = [np.zeros((max(n // G, 1), 32), dtype=np.uint8) for _ in range(2)]; ms = ctypes.c_float(0)
        _check(lib.otti_k_hash_ops(_ptr(ad), _ptr(de), _ptr(ts), n, _ptr(r), _ptr(gamma), G, rk, _ptr(o[0]), _ptr(o[1]), ctypes.byref(ms)))
        return o[0], o[1], ms.value

    @staticmethod
    def dot_many(E, Ps):
        """dev_dot_many: <E, P> for every polynomial of the list"""
        e, n = kernels._stack([E], "E"); p, _ = kernels._stack(Ps, "Ps", n)
        out = np.zeros((max(len(Ps), 1), 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_dot_many(_ptr(e), _ptr(p), len(Ps), n, _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def sum3(A, B, C):
        """dev_sum3: sum_i A[i] B[i] C[i] for every triple of the lists"""
        if not (len(A) == len(B) == len(C)):
            raise SpartanError(-21, "one A, B and C table per triple")
        a, n = kernels._stack(A, "A"); b, _ = kernels._stack(B, "B", n); c, _ = kernels._stack(C, "C", n)
        out = np.zeros((max(len(A), 1), 32), dtype=np.uint8); ms = ctypes.c_float(0)
        _check(lib.otti_k_sum3(_ptr(a), _ptr(b), _ptr(c), len(A), n, _ptr(out), ctypes.byref(ms)))
        return out, ms.value

    @staticmethod
    def poly_bound_chunks(Z, L, R, Lv_rest):
        """dev_poly_bound_chunks with m = len(Lv_rest) rows per chunk: (L / m, R, 32), or None when the launch function declines the geometry"""
        Z, lv = _scalars(Z, "Z"), _scalars(Lv_rest, "Lv_rest"); m = lv.shape[0]
        if Z.shape[0] != L * R:
            raise SpartanError(-21, "Z: L * R elements")
        out = np.zeros((max(L // max(m, 1), 1) * R, 32), dtype=np.uint8); ok = _i32(0); ms = ctypes.c_float(0)
        _check(lib.otti_k_poly_bound_chunks(_ptr(Z), L, R, _ptr(lv), m, _ptr(out), ctypes.byref(ok), ctypes.byref(ms)))
        return out.reshape(-1, R, 32) if ok.value else None


class DeviceArray:
    """(n, 32) field elements in HBM (otti_dev_alloc): operand of the device-pointer kernel entry points (otti_kd_*)"""

    def __init__(self, n, nbytes_each=32):
        self.n, self.each = n, nbytes_each
        p = _vp()
        _check(lib.otti_dev_alloc(max(1, n * nbytes_each), ctypes.byref(p)))
        self.ptr = p

    @classmethod
    def from_host(cls, a):
        a = _scalars(a, "a"); d = cls(a.shape[0])
        _check(lib.otti_dev_upload(d.ptr, _ptr(a), a.nbytes))
        return d

    def to_host(self, n=None):
        n = self.n if n is None else n
        out = np.zeros((n, self.each), dtype=np.uint8)
        _check(lib.otti_dev_download(_ptr(out), self.ptr, out.nbytes))
        return out

    def __del__(self):
        if getattr(self, "ptr", None):
            lib.otti_dev_free(self.ptr); self.ptr = None


class kernels_dev:
    """otti_kd_*: the same kernels on device pointers and a caller's stream (None = the library's stream of this thread)"""

    @staticmethod
    def stream_create():
        s = _vp(); _check(lib.otti_dev_stream_create(ctypes.byref(s))); return s

    @staticmethod
    def stream_sync(s):
        _check(lib.otti_dev_stream_sync(s))

    @staticmethod
    def stream_destroy(s):
        _check(lib.otti_dev_stream_destroy(s))

    @staticmethod
    def multiply_vec(inst, z, Az, Bz, Cz, stream=None):
        _check(lib.otti_kd_multiply_vec(inst._h, z.ptr, Az.ptr, Bz.ptr, Cz.ptr, stream))

    @staticmethod
    def check_sat(inst, z, bits, stream=None):
        """the satisfiability pass on a device vector z; bits: DeviceArray(ceil(num_cons / 64), 8).  Returns the number of failing constraints."""
        n = _u64(); _check(lib.otti_kd_check_sat(inst._h, z.ptr, bits.ptr, ctypes.byref(n), stream)); return n.value

    @staticmethod
    def eval_table_sparse(inst, eq_rx, rABC, out, stream=None):
        rABC = _scalars(rABC, "rABC"); _check(lib.otti_kd_eval_table_sparse(inst._h, eq_rx.ptr, _ptr(rABC), out.ptr, stream))

    @staticmethod
    def eq_evals(r, out, stream=None):
        r = _scalars(r, "r"); _check(lib.otti_kd_eq_evals(_ptr(r), r.shape[0], out.ptr, stream))

    @staticmethod
    def fold_top(Z, length, r, stream=None):
        r = _scalars(r, "r"); _check(lib.otti_kd_fold_top(Z.ptr, length, _ptr(r), stream))

    @staticmethod
    def fold_bot(Z, out, length, r, stream=None):
        r = _scalars(r, "r"); _check(lib.otti_kd_fold_bot(Z.ptr, out.ptr, length, _ptr(r), stream))

    @staticmethod
    def sc_cubic_round(A, B, C, D, length, stream=None):
        e = np.zeros((3, 32), dtype=np.uint8); _check(lib.otti_kd_sc_cubic_round(A.ptr, B.ptr, C.ptr, D.ptr, length, _ptr(e), stream)); return e

    @staticmethod
    def sc_cubic_fold_round(A, B, C, D, length, r, stream=None):
        r = _scalars(r, "r"); e = np.zeros((3, 32), dtype=np.uint8)
        _check(lib.otti_kd_sc_cubic_fold_round(A.ptr, B.ptr, C.ptr, D.ptr, length, _ptr(r), _ptr(e), stream)); return e

    @staticmethod
    def sc_quad_round(A, B, length, stream=None):
        e = np.zeros((2, 32), dtype=np.uint8); _check(lib.otti_kd_sc_quad_round(A.ptr, B.ptr, length, _ptr(e), stream)); return e

    @staticmethod
    def sc_quad_fold_round(A, B, length, r, stream=None):
        r = _scalars(r, "r"); e = np.zeros((2, 32), dtype=np.uint8)
        _check(lib.otti_kd_sc_quad_fold_round(A.ptr, B.ptr, length, _ptr(r), _ptr(e), stream)); return e

    @staticmethod
    def msm_rows(gens, Z, L, R, blinds, out32, stream=None):
        _check(lib.otti_kd_msm_rows(gens._h, Z.ptr, L, R, blinds.ptr, out32.ptr, stream))
