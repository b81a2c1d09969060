"""recursive-stwo_amd — host-side binding of the MI355X-native batch verifier.

This package is plumbing only: it loads ``csrc/librsv_hip.so`` (the C-ABI of
``include/rsv.h``) with ctypes and exposes the same entry points to Python,
either on host ``bytes``/numpy arrays (copied to the device by the library) or
on torch tensors that already live in HBM (``Context``).  There is no CPU
implementation here: if the library is missing, or no HIP device is usable,
every call raises.

Reference items mirrored (values only; see include/rsv.h for file:line):
  poseidon2_permute        primitives/poseidon31/src/implementation.rs:108-149
  half_permute             Poseidon2HalfVar::permute, primitives/poseidon31/src/lib.rs:282-423
  poseidon2_emulated       poseidon_permute_emulated (gate values), primitives/poseidon31/src/emulated.rs:80-221
  hash_node                Poseidon31MerkleHasherVar, primitives/merkle/src/lib.rs:9-181
  merkle_path_root         SinglePathMerkleProofVar::verify, components/recursive/data_structures/src/lib.rs:315-354
  transcript               FiatShamirResults::compute, components/recursive/fiat_shamir/src/lib.rs:31-176
  verify_batch             FiatShamirResults/CompositionCheck/AnswerResults/FoldingResults::compute
"""
from __future__ import annotations

import ctypes
import weakref
import os
from typing import Iterable, Optional, Sequence

import numpy as np

P = 0x7FFFFFFF
_HERE = os.path.dirname(os.path.abspath(__file__))
# (rsvload.load_package(lib_path=...) names a diagnostic build explicitly; nothing here reads the environment)
LIB_PATH = globals().get("_LIB_PATH_OVERRIDE") or os.path.join(_HERE, "csrc", "librsv_hip.so")

REASONS = ["ok", "parse", "pow", "logup", "composition", "dup_query", "merkle_t0", "merkle_t1",
           "merkle_t2", "merkle_t3", "fri_first", "fri_inner", "fri_last"]

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)


class RsvError(RuntimeError):
    def __init__(self, code: int, what: str):
        names = {-1: "RSV_E_NULL", -2: "RSV_E_SIZE", -3: "RSV_E_DEVICE", -4: "RSV_E_CAP", -5: "RSV_E_RANGE", -6: "RSV_E_UNAVAILABLE"}
        super().__init__(f"{what}: {names.get(code, code)}")
        self.code = code


class PcsConfig(ctypes.Structure):
    """stwo PcsConfig{pow_bits, FriConfig::new(log_last_layer_degree_bound, log_blowup_factor, n_queries)}."""
    _fields_ = [("pow_bits", ctypes.c_uint32), ("log_blowup_factor", ctypes.c_uint32),
                ("log_last_layer_degree_bound", ctypes.c_uint32), ("n_queries", ctypes.c_uint32)]


class CfgSet(ctypes.Structure):  # rsv_cfg_set
    _fields_ = [("cfgs", ctypes.POINTER(PcsConfig)), ("n_cfgs", ctypes.c_uint32), ("cfg_of", ctypes.c_void_p)]


MAX_CFGS = 16  # RSV_MAX_CFGS


class PreparedCfg:
    """An rsv_cfg_set ready to pass by reference: keeps the config array (and the cfg_of buffer: a numpy array for
    the host entry points, a torch tensor in HBM for Context methods) alive."""

    def __init__(self, cfgs: Sequence[PcsConfig], cfg_of=None):
        if not 1 <= len(cfgs) <= MAX_CFGS:
            raise ValueError(f"1..{MAX_CFGS} configurations")
        self.arr = (PcsConfig * len(cfgs))(*[PcsConfig(c.pow_bits, c.log_blowup_factor, c.log_last_layer_degree_bound,
                                                       c.n_queries) for c in cfgs])
        self.cfg_of = cfg_of
        if cfg_of is None:
            ptr = None
        elif isinstance(cfg_of, np.ndarray):
            ptr = cfg_of.ctypes.data
        else:
            ptr = cfg_of.data_ptr()  # torch tensor
        self.struct = CfgSet(ctypes.cast(self.arr, ctypes.POINTER(PcsConfig)), len(cfgs), ptr)

    def ref(self):
        return ctypes.byref(self.struct)


def _cfg_key(c) -> tuple:
    return (int(c.pow_bits), int(c.log_blowup_factor), int(c.log_last_layer_degree_bound), int(c.n_queries))


def prepare_cfg(cfg, n: int, to_device=None) -> PreparedCfg:
    """cfg: one PcsConfig (every proof must carry it), or a sequence of n PcsConfig (one per proof; deduplicated into
    at most MAX_CFGS distinct configurations + a per-proof index), or a PreparedCfg.  The configuration is REQUIRED:
    the verifier never trusts the words serialized in a proof (include/rsv.h, rsv_cfg_set).
    to_device: callable numpy uint8 array -> device tensor (Context methods), None for the host entry points."""
    if isinstance(cfg, PreparedCfg):
        return cfg
    if cfg is None:
        raise TypeError("a PcsConfig (or one per proof) is required: the verifier does not trust the configuration "
                        "words serialized in a proof")
    if isinstance(cfg, PcsConfig) or hasattr(cfg, "pow_bits"):
        return PreparedCfg([cfg])
    per_proof = list(cfg)
    if len(per_proof) != n:
        raise ValueError("one configuration per proof expected")
    table, index = [], {}
    cfg_of = np.zeros(n, np.uint8)
    for i, c in enumerate(per_proof):
        k = _cfg_key(c)
        if k not in index:
            index[k] = len(table)
            table.append(c)
        cfg_of[i] = index[k]
    if len(table) <= 1:
        return PreparedCfg(table or [PcsConfig(0, 0, 0, 0)])
    return PreparedCfg(table, to_device(cfg_of) if to_device else cfg_of)


class PublicInput(ctypes.Structure):
    _fields_ = [("idx", ctypes.c_uint32), ("value", ctypes.c_uint32 * 4)]


class HintsOut(ctypes.Structure):  # rsv_hints_out
    _fields_ = [("n_queries", ctypes.c_uint32), ("max_log", ctypes.c_uint32), ("n_inner", ctypes.c_uint32),
                ("d_transcript", ctypes.c_void_p), ("d_trace_sib", ctypes.c_void_p), ("d_trace_pos", ctypes.c_void_p),
                ("d_trace_cols", ctypes.c_void_p), ("d_fri_sib", ctypes.c_void_p), ("d_fri_cols", ctypes.c_void_p),
                ("d_fri_folded", ctypes.c_void_p), ("d_query_values", ctypes.c_void_p),
                ("d_flow", ctypes.c_void_p), ("d_flow_swap", ctypes.c_void_p), ("d_flow_count", ctypes.c_void_p),
                ("flow_stride", ctypes.c_uint32), ("d_accept_bitmap", ctypes.c_void_p), ("d_accept_count", ctypes.c_void_p)]


class WitnessShape(ctypes.Structure):  # rsv_witness_shape
    _fields_ = [(k, ctypes.c_uint32) for k in ("log_size_plonk", "log_size_poseidon", "pow_bits", "log_blowup", "log_last", "n_queries",
                                               "n_inner", "flow_count", "copies")]


class CommitGroup(ctypes.Structure):  # rsv_commit_group
    _fields_ = [("log_size", ctypes.c_uint32), ("n_cols", ctypes.c_uint32), ("d_cols", ctypes.c_void_p), ("proof_stride", ctypes.c_uint64),
                ("d_coeffs", ctypes.c_void_p), ("d_lde", ctypes.c_void_p)]


class FriGroupPoints(ctypes.Structure):  # rsv_fri_group_points
    _fields_ = [("col_lo", ctypes.c_uint32 * 4), ("col_hi", ctypes.c_uint32 * 4)]


class Shard(ctypes.Structure):  # rsv_shard
    _fields_ = [("d_blob", ctypes.c_void_p), ("d_offsets", ctypes.c_void_p), ("n", ctypes.c_size_t), ("d_cfg_of", ctypes.c_void_p),
                ("d_accept", ctypes.c_void_p), ("d_reason", ctypes.c_void_p)]


class ProofList(ctypes.Structure):  # rsv_proof_list
    _fields_ = [("d_items", ctypes.c_void_p), ("stride", ctypes.c_size_t), ("d_count", ctypes.c_void_p), ("count_stride", ctypes.c_size_t),
                ("cap", ctypes.c_uint32)]


class ProofParts(ctypes.Structure):  # rsv_proof_parts
    _fields_ = [(k, ctypes.c_uint32) for k in ("log_size_plonk", "log_size_poseidon", "pow_bits", "log_blowup", "log_last", "n_queries",
                                               "n_layers")] + \
               [(k, ctypes.c_void_p) for k in ("d_sums", "d_roots", "d_root3", "d_samples", "d_samples3", "d_nonce", "d_fri_roots", "d_last_poly")] + \
               [("values", ProofList * 4), ("witness", ProofList * 4), ("fri_witness", ProofList), ("fri_hash_witness", ProofList)]


TRANSCRIPT_WORDS = 284  # RSV_TRANSCRIPT_WORDS
EXCHANGE_ID_BYTES = 128  # RSV_EXCHANGE_ID_BYTES


def _load() -> ctypes.CDLL:
    # PyTorch-ROCm bundles its own HIP runtime (same SONAME as /opt/rocm's).  Import torch first so that
    # the process holds ONE runtime and the tensors torch allocates are visible to this library's stream.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    sz = ctypes.c_size_t
    vp = ctypes.c_void_p
    sig = {
        "rsv_abi_version": (ctypes.c_int, []),
        "rsv_device_count": (ctypes.c_int, []),
        "rsv_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(vp)]),
        "rsv_ctx_destroy": (None, [vp]),
        "rsv_ctx_synchronize": (ctypes.c_int, [vp]),
        "rsv_ctx_stream": (vp, [vp]),
        "rsv_ctx_set_option": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_longlong]),
        "rsv_poseidon2_permute": (ctypes.c_int, [_u32p, _u32p, sz, ctypes.c_int]),
        "rsv_poseidon2_permute_dev": (ctypes.c_int, [vp, vp, vp, sz, vp]),
        "rsv_ctx_wait_stream": (ctypes.c_int, [vp, vp]),
        "rsv_stream_wait_ctx": (ctypes.c_int, [vp, vp]),
        "rsv_poseidon2_half_permute": (ctypes.c_int, [_u32p, _u32p, _u8p, _u32p, _u32p, sz, ctypes.c_int]),
        "rsv_poseidon2_emulated": (ctypes.c_int, [_u32p, _u32p, _u8p, _u32p, sz, ctypes.c_int]),
        "rsv_poseidon2_emulated_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, sz, vp]),
        "rsv_merkle_hash_node": (ctypes.c_int, [_u32p, _u32p, _u32p, sz, _u32p, sz, ctypes.c_int]),
        "rsv_merkle_path_root": (ctypes.c_int, [_u32p, _u32p, _u32p, _u32p, ctypes.c_uint32, _u32p, sz, ctypes.c_int]),
        "rsv_transcript": (ctypes.c_int, [_u8p, sz, _u32p, sz, ctypes.c_int]),
        "rsv_verify_batch": (ctypes.c_int, [_u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput),
                                            sz, _u8p, _u8p, ctypes.c_int]),
        "rsv_verify_batch_dev": (ctypes.c_int, [vp, vp, vp, sz, ctypes.POINTER(CfgSet),
                                                ctypes.POINTER(PublicInput), sz, vp, vp]),
        "rsv_verify_batch_inputs_dev": (ctypes.c_int, [vp, vp, vp, sz, ctypes.POINTER(CfgSet), vp, sz, vp, vp]),
        "rsv_verify_batch_inputs": (ctypes.c_int, [_u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, _u8p, _u8p,
                                                   ctypes.c_int]),
        "rsv_verify_hints_inputs_dev": (ctypes.c_int, [vp, vp, vp, sz, ctypes.POINTER(CfgSet), vp, sz, ctypes.POINTER(HintsOut), vp, vp]),
        "rsv_public_input_sum_dev": (ctypes.c_int, [vp, vp, sz, sz, vp, vp, vp]),
        "rsv_statement_digest_dev": (ctypes.c_int, [vp, vp, sz, sz, sz, vp, vp]),
        "rsv_circuit_program_num_input": (ctypes.c_int, [vp, _u32p]),
        "rsv_circuit_inputs_dev": (ctypes.c_int, [vp, vp, vp, sz, vp]),
        "rsv_accept_bitmap_dev": (ctypes.c_int, [vp, vp, sz, vp, vp]),
        "rsv_trace_paths_dev": (ctypes.c_int, [vp, vp, vp, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, ctypes.c_uint32,
                                               ctypes.c_uint32, vp, vp, vp, vp]),
        "rsv_verify_hints_dev": (ctypes.c_int, [vp, vp, vp, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, ctypes.POINTER(HintsOut), vp, vp]),
        "rsv_field_op": (ctypes.c_int, [ctypes.c_int, _u32p, _u32p, _u32p, sz, ctypes.c_int]),
        "rsv_domain_points": (ctypes.c_int, [ctypes.c_uint32, _u32p, _u32p, sz, ctypes.c_int]),
        "rsv_line_eval": (ctypes.c_int, [_u32p, ctypes.c_uint32, _u32p, _u32p, sz, ctypes.c_int]),
        "rsv_oods_eval": (ctypes.c_int, [_u32p, _u32p, _u32p, sz, ctypes.c_int]),
        "rsv_last_layer_check": (ctypes.c_int, [_u32p, ctypes.c_uint32, _u32p, _u32p, _u8p, sz, ctypes.c_int]),
        "rsv_verify_batch_host": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_void_p), _u64p, sz, ctypes.POINTER(CfgSet),
                                                 ctypes.POINTER(PublicInput), sz, _u8p, _u8p]),
        "rsv_verify_hints": (ctypes.c_int, [_u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, ctypes.POINTER(HintsOut), _u8p, _u8p,
                                            ctypes.c_int]),
        "rsv_transcript_batch": (ctypes.c_int, [_u8p, _u64p, sz, ctypes.POINTER(CfgSet), _u32p, ctypes.c_int]),
        "rsv_poseidon_flow_count": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(PcsConfig), _u32p]),
        "rsv_fri_paths_dev": (ctypes.c_int, [vp, vp, vp, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, ctypes.c_uint32,
                                             ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp, vp]),
        "rsv_fri_paths": (ctypes.c_int, [_u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_uint32, _u32p, _u32p, _u8p, _u8p, ctypes.c_int]),
        "rsv_trace_paths": (ctypes.c_int, [_u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, ctypes.c_uint32,
                                           ctypes.c_uint32, _u32p, _u32p, _u8p, _u8p, ctypes.c_int]),
        "rsv_last_stage_times": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_float),
                                                ctypes.c_int]),
        "rsv_witness_program_create": (ctypes.c_int, [_u32p, sz, _u32p, sz, ctypes.c_uint32, ctypes.POINTER(WitnessShape), ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_void_p)]),
        "rsv_witness_program_destroy": (None, [vp]),
        "rsv_witness_program_build": (ctypes.c_int, [_u8p, sz, ctypes.POINTER(PcsConfig), ctypes.POINTER(PublicInput), sz, ctypes.c_uint32,
                                                     _u8p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
        "rsv_witness_program_build_inputs": (ctypes.c_int, [_u8p, sz, ctypes.POINTER(PcsConfig), ctypes.POINTER(PublicInput), sz, sz,
                                                            ctypes.c_uint32, _u8p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
        "rsv_witness_program_inputs": (ctypes.c_int, [vp, _u32p, _u32p, _u32p]),
        "rsv_witness_program_build_inputs_hashed": (ctypes.c_int, [_u8p, sz, ctypes.POINTER(PcsConfig), ctypes.POINTER(PublicInput), sz, sz,
                                                                   ctypes.c_uint32, _u8p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
        "rsv_witness_program_statement": (ctypes.c_int, [vp, _u32p, _u32p, _u32p]),
        "rsv_witness_eval_inputs_dev": (ctypes.c_int, [vp, vp, vp, vp, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, vp, sz, vp, vp,
                                                       vp, vp, vp]),
        "rsv_witness_eval_inputs": (ctypes.c_int, [vp, _u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz,
                                                   ctypes.POINTER(PublicInput), sz, _u32p, _u32p, _u8p, _u8p, _u8p, ctypes.c_int]),
        "rsv_witness_eval_groups_inputs_dev": (ctypes.c_int, [vp, vp, vp, vp, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, vp, sz,
                                                              vp, vp, vp, vp, vp, vp]),
        "rsv_witness_program_info": (ctypes.c_int, [vp, _u32p, _u32p, ctypes.POINTER(WitnessShape)]),
        "rsv_witness_program_export": (ctypes.c_int, [vp, _u32p, _u32p, _u32p]),
        "rsv_witness_program_gates": (ctypes.c_int, [vp, _u32p, _u32p, _u32p, _u32p]),
        "rsv_witness_scratch_bytes": (ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
        "rsv_witness_eval_dev": (ctypes.c_int, [vp, vp, vp, vp, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, vp, vp, vp, vp, vp]),
        "rsv_witness_eval": (ctypes.c_int, [vp, _u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, _u32p, _u32p, _u8p,
                                            _u8p, _u8p, ctypes.c_int]),
        "rsv_witness_eval_groups_dev": (ctypes.c_int, [vp, vp, vp, vp, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, vp, vp, vp, vp, vp,
                                                       vp]),
        "rsv_witness_group_scratch_bytes": (ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
        "rsv_witness_trace_groups_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "rsv_trace_log_sizes": (ctypes.c_int, [sz, sz, _u32p, _u32p]),
        "rsv_trace_preprocessed": (ctypes.c_int, [_u32p, sz, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p]),
        "rsv_trace_preprocessed_inputs": (ctypes.c_int, [_u32p, sz, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u32p, _u32p]),
        "rsv_circuit_program_create": (ctypes.c_int, [_u32p, sz, _u32p, sz, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_void_p)]),
        "rsv_circuit_check_dev": (ctypes.c_int, [vp, vp, vp, sz, vp, vp]),
        "rsv_circuit_flow_dev": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, vp, vp]),
        "rsv_circuit_program_create_eval": (ctypes.c_int, [_u32p, sz, _u32p, sz, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, _u32p, sz, _u32p,
                                                           ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
        "rsv_circuit_eval_info": (ctypes.c_int, [vp, _u32p, _u32p, _u32p]),
        "rsv_circuit_eval_export": (ctypes.c_int, [vp, _u32p, _u32p, _u32p, _u32p]),
        "rsv_circuit_eval_scratch_bytes": (ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
        "rsv_circuit_eval_dev": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, vp, vp, vp]),
        "rsv_witness_trace_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "rsv_witness_trace": (ctypes.c_int, [vp, _u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, _u32p, _u32p, _u32p,
                                             _u8p, _u8p, ctypes.c_int]),
        "rsv_witness_interaction_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "rsv_witness_interaction": (ctypes.c_int, [vp, _u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, _u32p, _u32p,
                                                   _u32p, _u32p, _u8p, _u8p, _u8p, ctypes.c_int]),
        "rsv_commit_tree_dev": (ctypes.c_int, [vp, ctypes.POINTER(CommitGroup), sz, sz, ctypes.c_uint32, vp, vp]),
        "rsv_witness_commit_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp]),
        "rsv_commit_tree_cap_dev": (ctypes.c_int, [vp, ctypes.POINTER(CommitGroup), sz, sz, ctypes.c_uint32, vp, vp, vp]),
        "rsv_witness_commit_caps_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rsv_decommit_sizes": (ctypes.c_int, [ctypes.POINTER(CommitGroup), sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(sz),
                                              ctypes.POINTER(sz)]),
        "rsv_decommit_tree_dev": (ctypes.c_int, [vp, ctypes.POINTER(CommitGroup), sz, sz, ctypes.c_uint32, vp, vp, ctypes.c_uint32, ctypes.c_int,
                                                 vp, vp, vp, vp, vp]),
        "rsv_witness_decommit_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp, ctypes.c_uint32, vp, vp, vp,
                                                    vp, vp]),
        "rsv_sample_tree_dev": (ctypes.c_int, [vp, ctypes.POINTER(CommitGroup), sz, sz, vp, ctypes.c_int, vp, ctypes.c_uint32, vp]),
        "rsv_witness_sample_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
        "rsv_composition_log_size": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
        "rsv_composition_dev": (ctypes.c_int, [vp, ctypes.c_uint32, ctypes.c_uint32] + [vp, ctypes.c_uint64] * 6 + [vp, vp, vp, sz, vp, vp]),
        "rsv_witness_tree3_dev": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rsv_fri_sizes": (ctypes.c_int, [ctypes.c_uint32] * 4 + [_u32p, _u32p, _u32p, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "rsv_fri_quotients_dev": (ctypes.c_int, [vp, ctypes.POINTER(CommitGroup), ctypes.POINTER(FriGroupPoints), sz, sz, ctypes.c_uint32, vp,
                                                 ctypes.c_int, vp, ctypes.c_uint32, vp, vp, vp]),
        "rsv_fri_commit_dev": (ctypes.c_int, [vp, vp, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp, vp]),
        "rsv_witness_fri_dev": (ctypes.c_int, [vp] * 9 + [sz, ctypes.c_uint32, ctypes.c_uint32] + [vp] * 12),
        "rsv_pow_grind_dev": (ctypes.c_int, [vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, sz, vp, vp, vp]),
        "rsv_draw_queries_dev": (ctypes.c_int, [vp, sz, vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]),
        "rsv_fri_open_sizes": (ctypes.c_int, [_u32p, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "rsv_fri_open_dev": (ctypes.c_int, [vp, vp, vp, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, sz, vp, vp, ctypes.c_uint32, vp, vp, vp, vp]),
        "rsv_fri_cap_sizes": (ctypes.c_int, [_u32p, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "rsv_fri_commit_cap_dev": (ctypes.c_int, [vp, vp, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint32, vp]),
        "rsv_witness_fri_caps_dev": (ctypes.c_int, [vp] * 9 + [sz, ctypes.c_uint32, ctypes.c_uint32] + [vp] * 12 + [ctypes.c_uint32, vp]),
        "rsv_fri_commit_tail_dev": (ctypes.c_int, [vp, vp, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, sz, vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint32, vp,
                                                   ctypes.c_uint32]),
        "rsv_witness_fri_tail_dev": (ctypes.c_int, [vp] * 9 + [sz, ctypes.c_uint32, ctypes.c_uint32] + [vp] * 12 + [ctypes.c_uint32, vp, ctypes.c_uint32]),
        "rsv_fri_open_cap_dev": (ctypes.c_int, [vp, vp, vp, _u32p, sz, ctypes.c_uint32, ctypes.c_uint32, sz, vp, vp, ctypes.c_uint32, vp, vp, vp, vp,
                                                ctypes.c_uint32, vp]),
        "rsv_proof_bytes": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, _u32p, ctypes.POINTER(sz)]),
        "rsv_proof_pack_dev": (ctypes.c_int, [vp, ctypes.POINTER(ProofParts), sz, vp, vp, sz, vp]),
        "rsv_witness_commit": (ctypes.c_int, [vp, _u8p, _u64p, sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz, ctypes.c_uint32,
                                              _u32p, _u32p, _u32p, _u8p, _u8p, _u8p, ctypes.c_int]),
        "rsv_host_alloc": (ctypes.c_int, [sz, ctypes.POINTER(vp)]),
        "rsv_host_free": (None, [vp]),
        "rsv_shard_range": (None, [sz, sz, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "rsv_shard_plan": (ctypes.c_int, [_u64p, sz, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "rsv_cfg_check": (ctypes.c_int, [ctypes.POINTER(PcsConfig)]),
        "rsv_exchange_create_plan": (ctypes.c_int, [vp, _u8p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(vp)]),
        "rsv_exchange_assemble_plan": (ctypes.c_int, [sz, ctypes.POINTER(sz), ctypes.POINTER(sz), _u32p, _u8p, _u32p]),
        "rsv_multi_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), sz, ctypes.POINTER(vp)]),
        "rsv_multi_destroy": (None, [vp]),
        "rsv_multi_size": (sz, [vp]),
        "rsv_multi_ctx": (vp, [vp, sz]),
        "rsv_multi_verify_batch_host": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_void_p), _u64p, sz, ctypes.POINTER(CfgSet),
                                                       ctypes.POINTER(PublicInput), sz, _u8p, _u8p, _u32p, _u64p]),
        "rsv_multi_verify_batch_dev": (ctypes.c_int, [vp, ctypes.POINTER(Shard), sz, ctypes.POINTER(CfgSet), ctypes.POINTER(PublicInput), sz,
                                                      _u32p, _u64p]),
        "rsv_exchange_available": (ctypes.c_int, []),
        "rsv_exchange_rccl_version": (ctypes.c_int, []),
        "rsv_exchange_unique_id": (ctypes.c_int, [_u8p]),
        "rsv_exchange_create": (ctypes.c_int, [vp, _u8p, ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(vp)]),
        "rsv_exchange_destroy": (None, [vp]),
        "rsv_exchange_layout": (ctypes.c_int, [vp, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "rsv_exchange_run": (ctypes.c_int, [vp, vp, vp, vp]),
        "rsv_exchange_assemble": (ctypes.c_int, [sz, sz, _u32p, _u8p, _u32p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export what rsv.h declares
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()
EXPORTS = ["rsv_abi_version", "rsv_device_count", "rsv_ctx_create", "rsv_ctx_destroy", "rsv_ctx_synchronize",
           "rsv_ctx_stream", "rsv_ctx_set_option", "rsv_ctx_wait_stream", "rsv_stream_wait_ctx", "rsv_poseidon2_permute", "rsv_poseidon2_permute_dev", "rsv_poseidon2_half_permute",
           "rsv_poseidon2_emulated", "rsv_poseidon2_emulated_dev",
           "rsv_merkle_hash_node", "rsv_merkle_path_root", "rsv_transcript", "rsv_verify_batch",
           "rsv_verify_batch_dev", "rsv_accept_bitmap_dev", "rsv_last_stage_times", "rsv_trace_paths_dev",
           "rsv_trace_paths", "rsv_fri_paths_dev", "rsv_fri_paths", "rsv_verify_hints_dev", "rsv_verify_hints", "rsv_verify_batch_host", "rsv_field_op", "rsv_domain_points",
           "rsv_line_eval", "rsv_oods_eval", "rsv_last_layer_check",
           "rsv_transcript_batch", "rsv_poseidon_flow_count", "rsv_witness_program_create", "rsv_witness_program_destroy",
           "rsv_witness_program_build", "rsv_witness_program_info", "rsv_witness_program_export", "rsv_witness_program_gates",
           "rsv_witness_scratch_bytes", "rsv_witness_eval_dev", "rsv_witness_eval", "rsv_witness_eval_groups_dev",
           "rsv_witness_group_scratch_bytes", "rsv_witness_trace_groups_dev", "rsv_trace_log_sizes", "rsv_trace_preprocessed",
           "rsv_witness_trace_dev", "rsv_witness_trace", "rsv_witness_interaction_dev", "rsv_witness_interaction",
           "rsv_commit_tree_dev", "rsv_witness_commit_dev", "rsv_witness_commit",
           "rsv_commit_tree_cap_dev", "rsv_witness_commit_caps_dev", "rsv_decommit_sizes", "rsv_decommit_tree_dev", "rsv_witness_decommit_dev",
           "rsv_sample_tree_dev", "rsv_witness_sample_dev",
           "rsv_composition_log_size", "rsv_composition_dev", "rsv_witness_tree3_dev",
           "rsv_fri_sizes", "rsv_fri_quotients_dev", "rsv_fri_commit_dev", "rsv_witness_fri_dev",
           "rsv_pow_grind_dev", "rsv_draw_queries_dev", "rsv_fri_open_sizes", "rsv_fri_open_dev",
           "rsv_fri_cap_sizes", "rsv_fri_commit_cap_dev", "rsv_witness_fri_caps_dev", "rsv_fri_open_cap_dev",
           "rsv_fri_commit_tail_dev", "rsv_witness_fri_tail_dev",
           "rsv_proof_bytes", "rsv_proof_pack_dev",
           "rsv_trace_preprocessed_inputs", "rsv_circuit_program_create", "rsv_circuit_check_dev", "rsv_circuit_flow_dev",
           "rsv_circuit_program_create_eval", "rsv_circuit_eval_info", "rsv_circuit_eval_export", "rsv_circuit_eval_scratch_bytes",
           "rsv_circuit_eval_dev",
           "rsv_verify_batch_inputs_dev", "rsv_verify_batch_inputs", "rsv_verify_hints_inputs_dev", "rsv_public_input_sum_dev",
           "rsv_circuit_program_num_input", "rsv_circuit_inputs_dev",
           "rsv_witness_program_build_inputs", "rsv_witness_program_inputs", "rsv_witness_eval_inputs_dev", "rsv_witness_eval_inputs",
           "rsv_witness_eval_groups_inputs_dev", "rsv_statement_digest_dev", "rsv_witness_program_build_inputs_hashed",
           "rsv_witness_program_statement",
           "rsv_host_alloc", "rsv_host_free", "rsv_shard_range", "rsv_multi_create", "rsv_multi_destroy", "rsv_multi_size", "rsv_multi_ctx", "rsv_multi_verify_batch_host",
           "rsv_multi_verify_batch_dev", "rsv_exchange_available", "rsv_exchange_rccl_version", "rsv_exchange_unique_id",
           "rsv_exchange_create", "rsv_exchange_destroy", "rsv_exchange_layout", "rsv_exchange_run", "rsv_exchange_assemble",
           "rsv_shard_plan", "rsv_cfg_check", "rsv_exchange_create_plan", "rsv_exchange_assemble_plan"]


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RsvError(rc, what)


def _u32(a, shape=None) -> np.ndarray:
    arr = np.ascontiguousarray(a, dtype=np.uint32)
    if shape is not None:
        arr = arr.reshape(shape)
    return arr


def device_count() -> int:
    return lib.rsv_device_count()


#: rsv_option (include/rsv.h) by name, and the named values of the three-way knobs (0 is always "automatic")
OPTIONS = {"transcript_form": 1, "transcript_split": 2, "oods_form": 3, "qconst_form": 4, "plan_form": 5, "tree_cap": 6,
           "overlap_trees": 7, "ws_budget_mb": 8, "perm_wg_per_cu": 9, "host_chunk_mb": 10, "host_threads": 11, "debug_log": 12,
           "critical_chain": 13, "device_order": 14,
           "witness_layout": 16, "witness_small_max": 17, "witness_small_log": 18, "cap_top": 19, "witness_walk_log": 20, "flow_cap": 21, "pair_order": 22, "tree_pace": 23, "stage_times": 24, "query_form": 25, "cap_mid": 26,
           "circuit_eval_form": 30, "statement_row_max": 31, "ws_fill": 32}
#: the hint kinds of rsv_circuit_program_create_eval (RSV_HINT_*)
HINT_KINDS = {"input": 0, "copy": 1, "inv": 2, "inv_or_zero": 3, "qinv": 4, "cinv": 5, "coord": 6, "bit": 7}
OPTION_VALUES = {"auto": 0, "per_level": 1, "walk": 2, "row": 1, "lane": 2, "paced": 1, "unpaced": 2, "row16": 3, "whole": 1, "split": 2, "parallel": 1, "serial": 2, "on": 1, "off": 2, "device": 1, "host": 2,
                 "by_proof": 1, "by_variable": 2}


def _set_option(handle, name: str, value) -> None:
    v = OPTION_VALUES[value] if isinstance(value, str) else int(value)
    _check(lib.rsv_ctx_set_option(handle, OPTIONS[name], v), f"rsv_ctx_set_option({name}={value})")


def set_default_option(name: str, value) -> None:
    """Process default of a tuning / diagnostic knob (rsv_ctx_set_option with ctx = NULL): inherited by every context
    created afterwards, including the ones the host-pointer entry points create for themselves.  The library never reads
    the environment."""
    _set_option(None, name, value)


def make_inputs(inputs: Iterable) -> "ctypes.Array[PublicInput]":
    """[(idx, (a0, a1, b0, b1)), ...] -> PublicInput array (e.g. (1, 1), (2, i), (3, u))."""
    items = list(inputs)
    arr = (PublicInput * max(len(items), 1))()
    for k, (idx, val) in enumerate(items):
        arr[k].idx = idx
        for t in range(4):
            arr[k].value[t] = int(val[t])
    return arr


#: public inputs used by examples/multi-proofs/src/main.rs:49-57
STANDARD_INPUTS = [(1, (1, 0, 0, 0)), (2, (0, 1, 0, 0)), (3, (0, 0, 1, 0))]


def poseidon2_permute(states, device: int = 0) -> np.ndarray:
    s = _u32(states).reshape(-1, 16)
    out = np.empty_like(s)
    _check(lib.rsv_poseidon2_permute(s.ctypes.data_as(_u32p), out.ctypes.data_as(_u32p), s.shape[0], device),
           "rsv_poseidon2_permute")
    return out


F_QADD, F_QSUB, F_QMUL, F_QINV, F_MMUL, F_MINV, F_CMUL, F_CINV, F_QMULI, F_QMULU, F_QPOW = range(11)  # RSV_F_*


def field_op(op: int, a, b=None, device: int = 0) -> np.ndarray:
    """Batched M31 / CM31 / QM31 arithmetic probe (rsv_field_op): a, b are (n, 4) QM31 words."""
    x = _u32(a).reshape(-1, 4)
    y = None if b is None else _u32(b).reshape(-1, 4)
    out = np.empty_like(x)
    _check(lib.rsv_field_op(op, x.ctypes.data_as(_u32p), None if y is None else y.ctypes.data_as(_u32p),
                            out.ctypes.data_as(_u32p), x.shape[0], device), "rsv_field_op")
    return out


def domain_points(log_size: int, q, device: int = 0) -> np.ndarray:
    """(n, 2) circle-domain points of the query positions q at log_size (rsv_domain_points)."""
    qq = _u32(q).reshape(-1)
    out = np.empty((qq.size, 2), np.uint32)
    _check(lib.rsv_domain_points(log_size, qq.ctypes.data_as(_u32p), out.ctypes.data_as(_u32p), qq.size, device),
           "rsv_domain_points")
    return out


def line_eval(coeffs, x, device: int = 0) -> np.ndarray:
    """LinePolyVar::eval_at_point of one polynomial (2^k QM31 coefficients) at the points x: (n, 4)."""
    c = _u32(coeffs).reshape(-1, 4)
    log_n = int(c.shape[0]).bit_length() - 1
    if c.shape[0] != 1 << log_n:
        raise ValueError("coefficient count must be a power of two")
    xx = _u32(x).reshape(-1)
    out = np.empty((xx.size, 4), np.uint32)
    _check(lib.rsv_line_eval(c.ctypes.data_as(_u32p), log_n, xx.ctypes.data_as(_u32p), out.ctypes.data_as(_u32p), xx.size,
                             device), "rsv_line_eval")
    return out


def oods_eval(samples, params, device: int = 0) -> np.ndarray:
    """a10 probe (rsv_oods_eval): samples (n, 142, 4), params (n, 26) = lp, lq, plonk_sum, poseidon_sum, z, alpha,
    random_coeff, oods.x -> (n, 8): constraint accumulator | expected value."""
    sm = _u32(samples).reshape(-1, 142, 4)
    pr = _u32(params).reshape(-1, 26)
    out = np.empty((sm.shape[0], 8), np.uint32)
    _check(lib.rsv_oods_eval(sm.ctypes.data_as(_u32p), pr.ctypes.data_as(_u32p), out.ctypes.data_as(_u32p), sm.shape[0], device),
           "rsv_oods_eval")
    return out


def last_layer_check(coeffs, x, folded, device: int = 0) -> np.ndarray:
    """ok[i] = 1 iff LinePoly(coeffs)(x[i]) == folded[i] (rsv_last_layer_check; the RSV_R_FRI_LAST comparison)."""
    c = _u32(coeffs).reshape(-1, 4)
    log_n = int(c.shape[0]).bit_length() - 1
    xx = _u32(x).reshape(-1)
    f = _u32(folded).reshape(-1, 4)
    ok = np.zeros(xx.size, np.uint8)
    _check(lib.rsv_last_layer_check(c.ctypes.data_as(_u32p), log_n, xx.ctypes.data_as(_u32p), f.ctypes.data_as(_u32p),
                                    ok.ctypes.data_as(_u8p), xx.size, device), "rsv_last_layer_check")
    return ok


def half_permute(left, right, swap=None, device: int = 0):
    """Poseidon2HalfVar::permute: returns (rate, capacity), each (n, 8)."""
    l = _u32(left).reshape(-1, 8)
    r = _u32(right).reshape(-1, 8)
    n = l.shape[0]
    sw = None if swap is None else np.ascontiguousarray(swap, dtype=np.uint8)
    rate = np.empty((n, 8), np.uint32)
    cap = np.empty((n, 8), np.uint32)
    _check(lib.rsv_poseidon2_half_permute(l.ctypes.data_as(_u32p), r.ctypes.data_as(_u32p),
                                          None if sw is None else sw.ctypes.data_as(_u8p),
                                          rate.ctypes.data_as(_u32p), cap.ctypes.data_as(_u32p), n, device),
           "rsv_poseidon2_half_permute")
    return rate, cap


EMU_SWAP_ROWS, EMU_ROWS, EMU_STRIDE = 12, 413, 416  # RSV_EMU_SWAP_ROWS, RSV_EMU_ROWS, RSV_EMU_STRIDE


def poseidon2_emulated(left, right, swap=None, device: int = 0) -> np.ndarray:
    """Gate values of poseidon_permute_emulated for n permutations: (n, 416, 4) QM31 rows (rows 0..11 = the swap
    gates, zero for is_swap None; rows 409..412 = the output state; rows 413..415 zero padding).  swap: None or n bytes, 0 = None,
    1 = Some((false, _)), 2 = Some((true, _))."""
    l = _u32(left).reshape(-1, 8)
    r = _u32(right).reshape(-1, 8)
    n = l.shape[0]
    sw = None if swap is None else np.ascontiguousarray(swap, dtype=np.uint8)
    rows = np.empty((n, EMU_STRIDE, 4), np.uint32)
    _check(lib.rsv_poseidon2_emulated(l.ctypes.data_as(_u32p), r.ctypes.data_as(_u32p),
                                      None if sw is None else sw.ctypes.data_as(_u8p), rows.ctypes.data_as(_u32p), n,
                                      device), "rsv_poseidon2_emulated")
    return rows


def hash_node(children, cols, device: int = 0) -> np.ndarray:
    """Poseidon31MerkleHasher::hash_node for n nodes.  children = None or (left (n,8), right (n,8));
    cols = (n, n_cols) array (n_cols may be 0 when children are given)."""
    c = _u32(cols)
    if c.ndim == 1:
        c = c.reshape(1, -1)
    n, n_cols = c.shape
    out = np.empty((n, 8), np.uint32)
    if children is None:
        lp = rp = None
    else:
        l = _u32(children[0]).reshape(n, 8)
        r = _u32(children[1]).reshape(n, 8)
        lp, rp = l.ctypes.data_as(_u32p), r.ctypes.data_as(_u32p)
    _check(lib.rsv_merkle_hash_node(lp, rp, c.ctypes.data_as(_u32p) if n_cols else None, n_cols,
                                    out.ctypes.data_as(_u32p), n, device), "rsv_merkle_hash_node")
    return out


def merkle_path_root(query, siblings, cols, n_cols_at: Sequence[int], device: int = 0) -> np.ndarray:
    q = _u32(query).reshape(-1)
    n = q.shape[0]
    depth = len(n_cols_at) - 1
    sib = _u32(siblings).reshape(n, depth, 8) if depth else np.zeros((n, 0, 8), np.uint32)
    nca = _u32(n_cols_at)
    c = _u32(cols).reshape(n, int(nca.sum()))
    out = np.empty((n, 8), np.uint32)
    _check(lib.rsv_merkle_path_root(q.ctypes.data_as(_u32p), sib.ctypes.data_as(_u32p), c.ctypes.data_as(_u32p),
                                    nca.ctypes.data_as(_u32p), depth, out.ctypes.data_as(_u32p), n, device),
           "rsv_merkle_path_root")
    return out


def _parse_transcript(out: np.ndarray) -> dict:
    if out[0] == 1:
        return {"reason": "parse"}
    na, nq = int(out[1]), int(out[2])
    q = lambda o: tuple(int(x) for x in out[o:o + 4])
    return {
        "reason": REASONS[int(out[0])], "n_queries": nq, "log_size": int(out[3]),
        "z": q(4), "alpha": q(8), "random_coeff": q(12), "oods_t": q(16), "oods_x": q(20), "oods_y": q(24),
        "after_sampled_values_random_coeff": q(28), "pow_digest": [int(x) for x in out[32:40]],
        "fri_alphas": [q(40 + 4 * i) for i in range(na)],
        "raw_queries": [int(x) for x in out[40 + 4 * na:40 + 4 * na + nq]],
    }


def transcript(proof: bytes, device: int = 0) -> dict:
    b = np.frombuffer(proof, dtype=np.uint8)
    out = np.zeros(1024, np.uint32)
    _check(lib.rsv_transcript(b.ctypes.data_as(_u8p), len(proof), out.ctypes.data_as(_u32p), out.size, device),
           "rsv_transcript")
    return _parse_transcript(out)


def pack(proofs: Sequence[bytes]):
    """Concatenate proofs into (blob uint8[total], offsets uint64[n+1])."""
    offsets = np.zeros(len(proofs) + 1, np.uint64)
    if proofs:
        offsets[1:] = np.cumsum([len(p) for p in proofs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(proofs), dtype=np.uint8) if proofs else np.zeros(0, np.uint8)
    return blob, offsets


def make_inputs_per_proof(inputs_per_proof, n: int):
    """n lists of (idx, value) pairs of one length -> (PublicInput array [n * n_pi], n_pi)."""
    per = [list(x) for x in inputs_per_proof]
    if len(per) != n:
        raise ValueError("inputs_per_proof: one list of inputs per proof expected")
    n_pi = len(per[0]) if per else 0
    if any(len(x) != n_pi for x in per):
        raise ValueError("inputs_per_proof: every proof needs the same number of inputs")
    return make_inputs([item for x in per for item in x]), n_pi


def inputs_array(inputs_per_proof, n: int) -> np.ndarray:
    """The same as uint32[n, n_pi, 5] records (idx, value[4]): the layout Context.verify_batch takes in HBM as d_inputs."""
    arr, n_pi = make_inputs_per_proof(inputs_per_proof, n)
    return np.frombuffer(arr, dtype=np.uint32, count=5 * n * n_pi).reshape(n, n_pi, 5).copy()


def verify_batch(proofs: Sequence[bytes], cfg, inputs=STANDARD_INPUTS, device: int = 0, inputs_per_proof=None):
    """Verify a batch of serialized proofs on the GPU under the configuration(s) `cfg` (required: one PcsConfig, or
    one per proof).  inputs: the public inputs the whole batch shares; inputs_per_proof: instead, a list of n input lists of
    equal length, every proof its own (rsv_verify_batch_inputs).  Returns (accept uint8[n], reason uint8[n])."""
    blob, offsets = pack(proofs)
    n = len(proofs)
    accept = np.zeros(n, np.uint8)
    reason = np.zeros(n, np.uint8)
    pc = prepare_cfg(cfg, n)
    if inputs_per_proof is not None:
        pi, n_pi = make_inputs_per_proof(inputs_per_proof, n)
        _check(lib.rsv_verify_batch_inputs(blob.ctypes.data_as(_u8p), offsets.ctypes.data_as(_u64p), n, pc.ref(), pi, n_pi,
                                           accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), device), "rsv_verify_batch_inputs")
        return accept, reason
    pi = make_inputs(inputs)
    _check(lib.rsv_verify_batch(blob.ctypes.data_as(_u8p), offsets.ctypes.data_as(_u64p), n,
                                pc.ref(), pi, len(list(inputs)),
                                accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), device), "rsv_verify_batch")
    return accept, reason


def trace_paths(proofs: Sequence[bytes], cfg, n_queries: int, max_log: int, inputs=STANDARD_INPUTS, device: int = 0):
    """per-query authentication paths of the four commitment trees, transcript query order.
    Returns (sib uint32[n,4,n_queries,max_log,8], pos uint32[n,4,n_queries], accept, reason)."""
    blob, offsets = pack(proofs)
    n = len(proofs)
    sib = np.zeros((n, 4, n_queries, max_log, 8), np.uint32)
    pos = np.zeros((n, 4, n_queries), np.uint32)
    accept = np.zeros(n, np.uint8)
    reason = np.zeros(n, np.uint8)
    pi = make_inputs(inputs)
    _check(lib.rsv_trace_paths(blob.ctypes.data_as(_u8p), offsets.ctypes.data_as(_u64p), n, prepare_cfg(cfg, n).ref(), pi, len(list(inputs)),
                               n_queries, max_log, sib.ctypes.data_as(_u32p), pos.ctypes.data_as(_u32p),
                               accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), device), "rsv_trace_paths")
    return sib, pos, accept, reason


def transcript_batch(proofs: Sequence[bytes], cfg, device: int = 0) -> np.ndarray:
    """FiatShamirHints of every proof of a batch (any mix of shapes): uint32[n, TRANSCRIPT_WORDS], layout in rsv.h."""
    blob, offsets = pack(proofs)
    n = len(proofs)
    out = np.zeros((n, TRANSCRIPT_WORDS), np.uint32)
    _check(lib.rsv_transcript_batch(blob.ctypes.data_as(_u8p), offsets.ctypes.data_as(_u64p), n, prepare_cfg(cfg, n).ref(), out.ctypes.data_as(_u32p),
                                    device), "rsv_transcript_batch")
    return out


def poseidon_flow_count(log_size_plonk: int, log_size_poseidon: int, cfg) -> int:
    """Records in the PoseidonFlow of one proof of this shape (rsv_poseidon_flow_count)."""
    c = PcsConfig(cfg.pow_bits, cfg.log_blowup_factor, cfg.log_last_layer_degree_bound, cfg.n_queries)
    out = ctypes.c_uint32(0)
    _check(lib.rsv_poseidon_flow_count(log_size_plonk, log_size_poseidon, ctypes.byref(c), ctypes.byref(out)), "rsv_poseidon_flow_count")
    return int(out.value)


def poseidon_flow(proofs: Sequence[bytes], cfg, flow_stride: int, inputs=STANDARD_INPUTS, device: int = 0):
    """SURVEY 8f.1 (second half): the PoseidonFlow of the circuit that verifies each proof, from the verifying pass
    (rsv_verify_hints with d_flow).  Returns (flow uint32[n, flow_stride, 32], swap uint8[n, flow_stride],
    count uint32[n], accept, reason); record = left8 | right8 | out_rate8 | out_cap8."""
    blob, offsets = pack(proofs)
    n = len(proofs)
    flow = np.zeros((n, flow_stride, 32), np.uint32)
    swap = np.zeros((n, flow_stride), np.uint8)
    count = np.zeros(n, np.uint32)
    accept = np.zeros(n, np.uint8)
    reason = np.zeros(n, np.uint8)
    pi = make_inputs(inputs)
    ho = HintsOut(0, 0, 0, None, None, None, None, None, None, None, None, flow.ctypes.data, swap.ctypes.data, count.ctypes.data, flow_stride,
                  None, None)
    _check(lib.rsv_verify_hints(blob.ctypes.data_as(_u8p), offsets.ctypes.data_as(_u64p), n, prepare_cfg(cfg, n).ref(), pi, len(list(inputs)),
                                ctypes.byref(ho), accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), device), "rsv_verify_hints")
    return flow, swap, count, accept, reason


def hints(proofs: Sequence[bytes], cfg, n_queries: int, max_log: int, n_inner: int, flow_stride: int, inputs=STANDARD_INPUTS, device: int = 0):
    """Everything the reference's hint structs hold for a uniform batch, from one verifying pass (rsv_verify_hints on host
    buffers): dict of trace_sib, trace_pos, trace_cols, fri_sib, fri_cols, flow, flow_swap, accept, reason (layouts: rsv.h)."""
    blob, offsets = pack(proofs)
    n = len(proofs)
    out = {"trace_sib": np.zeros((n, 4, n_queries, max_log, 8), np.uint32), "trace_pos": np.zeros((n, 4, n_queries), np.uint32),
           "trace_cols": np.zeros((n, 4, n_queries, 64), np.uint32), "fri_sib": np.zeros((n, 1 + n_inner, n_queries, max_log, 8), np.uint32),
           "fri_cols": np.zeros((n, 1 + n_inner, n_queries, 3, 8), np.uint32), "flow": np.zeros((n, flow_stride, 32), np.uint32),
           "flow_swap": np.zeros((n, flow_stride), np.uint8), "accept": np.zeros(n, np.uint8), "reason": np.zeros(n, np.uint8)}
    pi = make_inputs(inputs)
    ho = HintsOut(n_queries, max_log, n_inner, None, out["trace_sib"].ctypes.data, out["trace_pos"].ctypes.data, out["trace_cols"].ctypes.data,
                  out["fri_sib"].ctypes.data, out["fri_cols"].ctypes.data, None, None, out["flow"].ctypes.data, out["flow_swap"].ctypes.data,
                  None, flow_stride, None, None)
    _check(lib.rsv_verify_hints(blob.ctypes.data_as(_u8p), offsets.ctypes.data_as(_u64p), n, prepare_cfg(cfg, n).ref(), pi, len(list(inputs)),
                                ctypes.byref(ho), out["accept"].ctypes.data_as(_u8p), out["reason"].ctypes.data_as(_u8p), device), "rsv_verify_hints")
    return out


class WitnessProgram:
    """A witness program resident on the device (rsv_witness_program).  WitnessProgram.build(proof, cfg, ...) runs the
    library's mirror of the reference's circuit gadgets over a template proof (rsv_witness_program_build);
    WitnessProgram(program) loads arrays made earlier (witness_program.Program, e.g. from a file)."""

    num_input = 3  # the recursion circuit allocates no public input, unless built with own inputs (build(n_fixed=...))
    stmt_flow = 0

    def __init__(self, program=None, device: int = 0, _handle=None):
        self._h = None
        if _handle is not None:
            self._h = _handle
        else:
            program._not_hashed("WitnessProgram(program)")
            sh = program.shape
            shape = WitnessShape(sh["lp"], sh["lq"], sh["pow_bits"], sh["blowup"], sh["log_last"], sh["nq"], sh["n_inner"], sh["flow_count"],
                                 sh["copies"])
            instr = np.ascontiguousarray(program.instr, dtype=np.uint32)
            levels = np.ascontiguousarray(program.level_offsets, dtype=np.uint32)
            h = ctypes.c_void_p()
            _check(lib.rsv_witness_program_create(instr.ctypes.data_as(_u32p), instr.shape[0], levels.ctypes.data_as(_u32p), len(levels) - 1,
                                                  program.n_vars, ctypes.byref(shape), device, ctypes.byref(h)), "rsv_witness_program_create")
            self._h = h
            self._flow_wires = program.flow_wires
        n_vars, n_levels = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self.shape = WitnessShape()
        _check(lib.rsv_witness_program_info(self._h, ctypes.byref(n_vars), ctypes.byref(n_levels), ctypes.byref(self.shape)),
               "rsv_witness_program_info")
        self.n_vars, self.n_levels = int(n_vars.value), int(n_levels.value)
        num_input = ctypes.c_uint32(0)
        if lib.rsv_circuit_program_num_input(self._h, ctypes.byref(num_input)) == 0:  # (a program made from instructions has no gate list)
            self.num_input = int(num_input.value)
        #: the invocations of the statement hash of a hashed program (build(hashed=True)), whose flow records follow the
        #: members' in the flow buffers; 0 for every other program
        self.stmt_flow = self.statement()[2]

    @classmethod
    def build(cls, proof: bytes, cfg, inputs=STANDARD_INPUTS, copies: int = 1, device: int = 0, set_walks=None, n_fixed=None,
              hashed: bool = False) -> "WitnessProgram":
        """set_walks: per copy, which of the four orders the reference's two HashSet walks took (rsv.h); default 0 for all.
        n_fixed: None — every input is a constant of the program (rsv_witness_program_build); else inputs[:n_fixed] are, and
        inputs[n_fixed:] are the proof's own: PublicInput variables 4 + c * n_own + k of the circuit
        (rsv_witness_program_build_inputs), whose values Context.witness(d_inputs=...) takes per proof.
        hashed (with n_fixed): the circuit's statement is the eight words of the digest of the own records
        (Context.statement_digest; rsv_witness_program_build_inputs_hashed): num_input = 11 whatever copies and n_own are."""
        if hashed and n_fixed is None:
            raise ValueError("hashed=True hashes the proof's own inputs: n_fixed is needed")
        b = np.frombuffer(proof, dtype=np.uint8)
        walks = None if set_walks is None else np.ascontiguousarray(set_walks, dtype=np.uint8)
        if walks is not None and len(walks) != copies:
            raise ValueError("set_walks: one entry per copy")
        c = PcsConfig(cfg.pow_bits, cfg.log_blowup_factor, cfg.log_last_layer_degree_bound, cfg.n_queries)
        pi = make_inputs(inputs)
        h = ctypes.c_void_p()
        wp = walks.ctypes.data_as(_u8p) if walks is not None else None
        if n_fixed is None:
            _check(lib.rsv_witness_program_build(b.ctypes.data_as(_u8p), len(proof), ctypes.byref(c), pi, len(list(inputs)), copies, wp, device,
                                                 ctypes.byref(h)), "rsv_witness_program_build")
        elif hashed:
            _check(lib.rsv_witness_program_build_inputs_hashed(b.ctypes.data_as(_u8p), len(proof), ctypes.byref(c), pi, len(list(inputs)), n_fixed,
                                                               copies, wp, device, ctypes.byref(h)), "rsv_witness_program_build_inputs_hashed")
        else:
            _check(lib.rsv_witness_program_build_inputs(b.ctypes.data_as(_u8p), len(proof), ctypes.byref(c), pi, len(list(inputs)), n_fixed, copies,
                                                        wp, device, ctypes.byref(h)), "rsv_witness_program_build_inputs")
        return cls(_handle=h)

    def statement(self):
        """-> (hashed, n_words, stmt_flow_count): whether the program's statement is the digest of the statements it verifies
        (build(hashed=True)), then 8 and the invocations of that hash, else zeros (rsv_witness_program_statement)."""
        hashed, n_words, count = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib.rsv_witness_program_statement(self._h, ctypes.byref(hashed), ctypes.byref(n_words), ctypes.byref(count)),
               "rsv_witness_program_statement")
        return bool(hashed.value), int(n_words.value), int(count.value)

    def inputs(self):
        """-> (n_fixed, n_own, idx uint32[n_own]): the records a built program was made for (rsv_witness_program_inputs)."""
        n_fixed, n_own = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib.rsv_witness_program_inputs(self._h, ctypes.byref(n_fixed), ctypes.byref(n_own), None), "rsv_witness_program_inputs")
        idx = np.zeros(n_own.value, np.uint32)
        _check(lib.rsv_witness_program_inputs(self._h, None, None, idx.ctypes.data_as(_u32p)), "rsv_witness_program_inputs")
        return int(n_fixed.value), int(n_own.value), idx

    def export(self):
        """-> witness_program.Program (instr, level_offsets, shape, flow_wires): what save / save_raw write and __init__ takes back."""
        instr = np.zeros((self.n_vars, 8), np.uint32)
        levels = np.zeros(self.n_levels + 1, np.uint32)
        s = self.shape
        wires = getattr(self, "_flow_wires", None)
        if wires is None:
            wires = np.zeros((s.copies * s.flow_count + self.stmt_flow, 5), np.uint32)
            _check(lib.rsv_witness_program_export(self._h, instr.ctypes.data_as(_u32p), levels.ctypes.data_as(_u32p), wires.ctypes.data_as(_u32p)),
                   "rsv_witness_program_export")
        else:
            _check(lib.rsv_witness_program_export(self._h, instr.ctypes.data_as(_u32p), levels.ctypes.data_as(_u32p), None),
                   "rsv_witness_program_export")
        shape = dict(zip(witness_program.SHAPE_KEYS, (s.log_size_plonk, s.log_size_poseidon, s.pow_bits, s.log_blowup, s.log_last, s.n_queries,
                                              s.n_inner, s.flow_count, s.copies)))
        return witness_program.Program(instr, levels, self.n_vars, shape, wires)

    def gates(self, variables=None):
        """The circuit's Plonk rows (rsv_witness_program_gates): uint32[n_rows, 6] = a_wire, b_wire, c_wire, op,
        poseidon_wire, enforce_c_m31 — the template's; with `variables` (uint32[n_vars, 4] of another proof of the shape) the
        rows whose op follows the witness are set for that proof.  Also returns witness_ops uint32[n, 3]."""
        n_rows, n_ops = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib.rsv_witness_program_gates(self._h, ctypes.byref(n_rows), ctypes.byref(n_ops), None, None), "rsv_witness_program_gates")
        rows = np.zeros((n_rows.value, 6), np.uint32)
        ops = np.zeros((n_ops.value, 3), np.uint32)
        _check(lib.rsv_witness_program_gates(self._h, None, None, rows.ctypes.data_as(_u32p), ops.ctypes.data_as(_u32p)), "rsv_witness_program_gates")
        if variables is not None:
            rows[ops[:, 0], 3] = np.where(variables[ops[:, 1], 0] != 0, ops[:, 2], 0)
        return rows, ops

    def trace_sizes(self):
        """(log_plonk, log_poseidon) of the circuit's components (rsv_trace_log_sizes of its gate rows and flow)."""
        rows, _ = self.gates()
        return trace_log_sizes(len(rows), self.shape.copies * self.shape.flow_count + self.stmt_flow)

    def preprocessed(self, variables=None):
        """The 10 Plonk and 40 Poseidon preprocessed columns (rsv_trace_preprocessed): uint32[10, 2^lp], uint32[40, 2^lq].
        With `variables` (uint32[n_vars, 4] of one proof of the shape) `op` is that proof's, as gates(variables) sets it."""
        rows, _ = self.gates(variables)
        return trace_preprocessed(rows, self.export().flow_wires, num_input=self.num_input)

    def close(self):
        if getattr(self, "_h", None):
            lib.rsv_witness_program_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def cfg(self) -> PcsConfig:
        s = self.shape
        return PcsConfig(s.pow_bits, s.log_blowup, s.log_last, s.n_queries)

    def scratch_bytes(self, n: int) -> int:
        out = ctypes.c_size_t(0)
        _check(lib.rsv_witness_scratch_bytes(self._h, n, ctypes.byref(out)), "rsv_witness_scratch_bytes")
        return int(out.value)

    def group_scratch_bytes(self, n_groups: int) -> int:
        out = ctypes.c_size_t(0)
        _check(lib.rsv_witness_group_scratch_bytes(self._h, n_groups, ctypes.byref(out)), "rsv_witness_group_scratch_bytes")
        return int(out.value)


class Circuit(WitnessProgram):
    """A caller's own Plonk-with-Poseidon circuit as the chain's program (rsv_circuit_program_create): gates uint32[n_rows, 6]
    = a_wire, b_wire, c_wire, op, poseidon_wire, enforce_c_m31 (unpadded), flow_wires uint32[n_flow, 5] = the wires of
    r1..r4 and the swap address, witness_ops uint32[n, 3] = (row, bit variable, constant) or None — the arrays
    WitnessProgram.gates() and export() return.  num_input is the reference's: 3 for the constants 1, i, j plus one per
    public input; the public inputs are variables 1 .. num_input.  It has no instructions: the witness is the caller's
    (Chain.load), and what evaluates the recursion circuit's refuses it.  With hints uint32[n_hints, 4] = (dst, kind, src,
    imm) — HINT_KINDS names the kinds —, flow_links uint32[n_flow, 2] or None and n_inputs it is made by
    rsv_circuit_program_create_eval and also holds an evaluation program: Chain.evaluate computes the witnesses on the
    device from their n_inputs free inputs (rsv.h has the rule by which every variable gets its definition)."""

    def __init__(self, gates, flow_wires, n_vars: int, num_input: int = 3, witness_ops=None, device: int = 0, hints=None, flow_links=None,
                 n_inputs: int = 0):
        self._h = None
        g, w = _u32(gates, (-1, 6)), _u32(flow_wires, (-1, 5))
        ops = _u32(witness_ops if witness_ops is not None else [], (-1, 3))
        h = ctypes.c_void_p()
        lead = (g.ctypes.data_as(_u32p), len(g), w.ctypes.data_as(_u32p), len(w), ops.ctypes.data_as(_u32p) if len(ops) else None, len(ops),
                n_vars, num_input)
        if hints is None:
            _check(lib.rsv_circuit_program_create(*lead, device, ctypes.byref(h)), "rsv_circuit_program_create")
        else:
            hi = _u32(hints, (-1, 4))
            links = None if flow_links is None else _u32(flow_links, (-1, 2))
            if links is not None and len(links) != len(w):
                raise ValueError("Circuit: flow_links needs one pair per invocation")
            _check(lib.rsv_circuit_program_create_eval(*lead, hi.ctypes.data_as(_u32p) if len(hi) else None, len(hi),
                                                       links.ctypes.data_as(_u32p) if links is not None else None, n_inputs, device,
                                                       ctypes.byref(h)), "rsv_circuit_program_create_eval")
            #: bool[n_flow, 2]: the input halves r1, r2 with neither a wire nor a link, which rsv_circuit_eval_dev reads from d_flow
            self.flow_free = (w[:, :2] == 0) & ((links if links is not None else np.zeros((len(w), 2), np.uint32)) == 0)
        self.num_input = num_input
        super().__init__(_handle=h)

    def eval_info(self):
        """(n_inputs, n_levels, n_instr) of the evaluation program (rsv_circuit_eval_info); RsvError where there is none."""
        out = [ctypes.c_uint32(0) for _ in range(3)]
        _check(lib.rsv_circuit_eval_info(self._h, *(ctypes.byref(x) for x in out)), "rsv_circuit_eval_info")
        return tuple(int(x.value) for x in out)

    def eval_export(self):
        """-> (instr uint32[n_instr, 8], level_offsets uint32[n_levels + 1], flow_order uint32[n_flow], flow_level_offsets
        uint32[n_levels + 1]): the evaluation program as compiled (rsv_circuit_eval_export)."""
        _, n_levels, n_instr = self.eval_info()
        instr, levels = np.zeros((n_instr, 8), np.uint32), np.zeros(n_levels + 1, np.uint32)
        order, flevels = np.zeros(self.shape.flow_count, np.uint32), np.zeros(n_levels + 1, np.uint32)
        _check(lib.rsv_circuit_eval_export(self._h, instr.ctypes.data_as(_u32p), levels.ctypes.data_as(_u32p), order.ctypes.data_as(_u32p),
                                           flevels.ctypes.data_as(_u32p)), "rsv_circuit_eval_export")
        return instr, levels, order, flevels

    def eval_scratch_bytes(self, n: int) -> int:
        out = ctypes.c_size_t(0)
        _check(lib.rsv_circuit_eval_scratch_bytes(self._h, n, ctypes.byref(out)), "rsv_circuit_eval_scratch_bytes")
        return int(out.value)

    def export(self):
        """-> witness_program.Program with no instructions: the shape and the flow wires."""
        s = self.shape
        wires = np.zeros((s.flow_count, 5), np.uint32)
        levels = np.zeros(1, np.uint32)
        _check(lib.rsv_witness_program_export(self._h, None, levels.ctypes.data_as(_u32p), wires.ctypes.data_as(_u32p)),
               "rsv_witness_program_export")
        shape = dict(zip(witness_program.SHAPE_KEYS, (s.log_size_plonk, s.log_size_poseidon, s.pow_bits, s.log_blowup, s.log_last, s.n_queries,
                                              s.n_inner, s.flow_count, s.copies)))
        return witness_program.Program(np.zeros((0, 8), np.uint32), levels, self.n_vars, shape, wires)


def _witness_batch(proofs: Sequence[bytes], program: WitnessProgram, inputs):
    """What the rsv_witness_* host forms share: their leading arguments (program, blob, offsets, n, cfg, pi, n_pi), n, and
    the accept and reason arrays they fill."""
    blob, offsets = pack(proofs)
    n = len(proofs)
    items = list(inputs)
    lead = (program._h, blob.ctypes.data_as(_u8p), offsets.ctypes.data_as(_u64p), n, prepare_cfg(program.cfg(), n).ref(), make_inputs(items),
            len(items))
    return lead, n, np.zeros(n, np.uint8), np.zeros(n, np.uint8)


def _own_records(d_inputs, n: int, what: str) -> None:
    """d_inputs has to be every proof's own records as the library reads them: a contiguous int32 tensor [n, n_own, 5] (a
    slice such as inputs()[:, 3:, :] needs .contiguous(); fewer rows than proofs would be read past the end)."""
    import torch
    if d_inputs.dtype != torch.int32 or d_inputs.dim() != 3 or d_inputs.shape[0] != n or d_inputs.shape[2] != 5 or not d_inputs.is_contiguous():
        raise ValueError(f"{what}: d_inputs has to be a contiguous int32 tensor of shape ({n}, n_own, 5), not {d_inputs.dtype} "
                         f"{tuple(d_inputs.shape)}{'' if d_inputs.is_contiguous() else ', not contiguous'}")


def witness_program_build(proof: bytes, cfg, inputs=STANDARD_INPUTS, copies: int = 1, device: int = 0, set_walks=None, n_fixed=None) -> WitnessProgram:
    """WitnessProgram.build: n_fixed = None makes every input a constant of the program; else inputs[n_fixed:] are the
    proof's own (rsv_witness_program_build_inputs)."""
    return WitnessProgram.build(proof, cfg, inputs, copies, device, set_walks, n_fixed)


def witness(proofs: Sequence[bytes], program: WitnessProgram, inputs=STANDARD_INPUTS, device: int = 0, with_flow: bool = False):
    """`variables` of the recursion circuit for every proof of a batch (rsv_witness_eval): uint32[n, n_vars, 4], accept, reason
    [, flow uint32[n, flow_count, 32], flow_swap uint8[n, flow_count] with with_flow]."""
    lead, n, accept, reason = _witness_batch(proofs, program, inputs)
    variables = np.zeros((n, program.n_vars, 4), np.uint32)
    flow = np.zeros((n, program.shape.flow_count, 32), np.uint32) if with_flow else None
    swap = np.zeros((n, program.shape.flow_count), np.uint8) if with_flow else None
    _check(lib.rsv_witness_eval(*lead, variables.ctypes.data_as(_u32p), flow.ctypes.data_as(_u32p) if with_flow else None,
                                swap.ctypes.data_as(_u8p) if with_flow else None, accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), device),
           "rsv_witness_eval")
    return (variables, accept, reason, flow, swap) if with_flow else (variables, accept, reason)


def trace_log_sizes(n_rows: int, n_flow: int):
    """(log_plonk, log_poseidon) of the next proof's two components for a circuit of n_rows gate rows and n_flow Poseidon
    invocations (rsv_trace_log_sizes)."""
    lp, lq = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _check(lib.rsv_trace_log_sizes(n_rows, n_flow, ctypes.byref(lp), ctypes.byref(lq)), "rsv_trace_log_sizes")
    return int(lp.value), int(lq.value)


def trace_preprocessed(gates, flow_wires, log_plonk=None, log_poseidon=None, num_input: int = 3):
    """The 10 Plonk and 40 Poseidon preprocessed columns of a circuit (rsv_trace_preprocessed_inputs): uint32[10, 2^lp],
    uint32[40, 2^lq], at trace_log_sizes' log sizes unless larger ones are given.  num_input: 3 plus the public inputs."""
    rows, wires = _u32(gates, (-1, 6)), _u32(flow_wires, (-1, 5))
    lp, lq = trace_log_sizes(len(rows), len(wires))
    lp, lq = lp if log_plonk is None else log_plonk, lq if log_poseidon is None else log_poseidon
    plonk = np.zeros((10, 1 << lp), np.uint32)
    poseidon = np.zeros((40, 1 << lq), np.uint32)
    _check(lib.rsv_trace_preprocessed_inputs(rows.ctypes.data_as(_u32p), len(rows), wires.ctypes.data_as(_u32p), len(wires), lp, lq, num_input,
                                             plonk.ctypes.data_as(_u32p), poseidon.ctypes.data_as(_u32p)), "rsv_trace_preprocessed_inputs")
    return plonk, poseidon


def witness_trace(proofs: Sequence[bytes], program: WitnessProgram, inputs=STANDARD_INPUTS, device: int = 0):
    """The trace columns of the recursion circuit for every proof of a batch (rsv_witness_trace): plonk uint32[n, 12, 2^lp],
    poseidon uint32[n, 48, 2^lq], ops uint32[n, n_witness_ops], accept, reason."""
    lead, n, accept, reason = _witness_batch(proofs, program, inputs)
    lp, lq = program.trace_sizes()
    n_ops = len(program.gates()[1])
    plonk = np.zeros((n, 12, 1 << lp), np.uint32)
    poseidon = np.zeros((n, 48, 1 << lq), np.uint32)
    ops = np.zeros((n, n_ops), np.uint32)
    _check(lib.rsv_witness_trace(*lead, plonk.ctypes.data_as(_u32p), poseidon.ctypes.data_as(_u32p), ops.ctypes.data_as(_u32p),
                                 accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), device), "rsv_witness_trace")
    return plonk, poseidon, ops, accept, reason


def _lookup_array(lookup, n):
    """(z, alpha) per proof -> uint32[n, 8]: one pair (two 4-tuples, or 8 words) for all proofs, or one per proof."""
    arr = np.asarray(lookup, dtype=np.int64).reshape(-1, 8)
    if arr.shape[0] == 1 and n != 1:
        arr = np.repeat(arr, n, axis=0)
    if arr.shape[0] != n:
        raise RsvError(-2, "witness_interaction: lookup must be one (z, alpha) or one per proof")
    return np.ascontiguousarray(arr % 0x7FFFFFFF, dtype=np.uint32)


def witness_interaction(proofs: Sequence[bytes], program: WitnessProgram, lookup, inputs=STANDARD_INPUTS, device: int = 0):
    """The interaction (logup) columns of the recursion circuit for every proof of a batch (rsv_witness_interaction), with the
    next proof's lookup elements `lookup` = (z, alpha) for all proofs or [n] of them: int_plonk uint32[n, 8, 2^lp],
    int_poseidon uint32[n, 8, 2^lq], sums uint32[n, 2, 4] (the Plonk and Poseidon claimed sums), ok, accept, reason."""
    lead, n, accept, reason = _witness_batch(proofs, program, inputs)
    lk = _lookup_array(lookup, n)
    lp, lq = program.trace_sizes()
    int_plonk = np.zeros((n, 8, 1 << lp), np.uint32)
    int_poseidon = np.zeros((n, 8, 1 << lq), np.uint32)
    sums = np.zeros((n, 2, 4), np.uint32)
    ok = np.zeros(n, np.uint8)
    _check(lib.rsv_witness_interaction(*lead, lk.ctypes.data_as(_u32p), int_plonk.ctypes.data_as(_u32p), int_poseidon.ctypes.data_as(_u32p),
                                       sums.ctypes.data_as(_u32p), ok.ctypes.data_as(_u8p), accept.ctypes.data_as(_u8p),
                                       reason.ctypes.data_as(_u8p), device), "rsv_witness_interaction")
    return int_plonk, int_poseidon, sums, ok, accept, reason


def witness_commit(proofs: Sequence[bytes], program: WitnessProgram, log_blowup: int, inputs=STANDARD_INPUTS, device: int = 0):
    """Trees 0, 1 and 2 of the next proof for every proof of a batch and the transcript draws between them
    (rsv_witness_commit): roots uint32[n, 3, 8], draws uint32[n, 12] (z, alpha, random_coeff), sums uint32[n, 2, 4], ok,
    accept, reason."""
    lead, n, accept, reason = _witness_batch(proofs, program, inputs)
    roots = np.zeros((n, 3, 8), np.uint32)
    draws = np.zeros((n, 12), np.uint32)
    sums = np.zeros((n, 2, 4), np.uint32)
    ok = np.zeros(n, np.uint8)
    _check(lib.rsv_witness_commit(*lead, log_blowup, roots.ctypes.data_as(_u32p), draws.ctypes.data_as(_u32p), sums.ctypes.data_as(_u32p),
                                  ok.ctypes.data_as(_u8p), accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), device),
           "rsv_witness_commit")
    return roots, draws, sums, ok, accept, reason


def commit_groups(groups):
    """[{log_size, d_cols, n_cols (default: d_cols.shape[-2]), proof_stride (default: n_cols << log_size), d_coeffs, d_lde}]
    (torch tensors or None) -> a ctypes rsv_commit_group array."""
    arr = (CommitGroup * max(len(groups), 1))()
    for k, g in enumerate(groups):
        cols = g.get("d_cols")
        n_cols = g.get("n_cols", cols.shape[-2] if cols is not None and cols.dim() >= 2 else 1)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        arr[k] = CommitGroup(g["log_size"], n_cols, ptr(cols), g.get("proof_stride", n_cols << g["log_size"]), ptr(g.get("d_coeffs")),
                             ptr(g.get("d_lde")))
    return arr


CAP_NONE, CAP_WRITE, CAP_READ = 0, 1, 2  # rsv_cap_mode
SAMPLE_COLUMNS, SAMPLE_COEFFS = 0, 1  # rsv_sample_source
MAX_SAMPLE_POINTS = 4  # RSV_MAX_SAMPLE_POINTS


def decommit_sizes(groups, log_blowup: int, n_queries: int):
    """rsv_decommit_sizes: (values_cap in words, witness_cap in nodes) per proof of rsv_decommit_tree_dev's outputs; groups
    as commit_groups() takes them, or (log_size, n_cols) pairs.  Host arithmetic."""
    if groups and not isinstance(groups[0], dict):
        arr = (CommitGroup * len(groups))(*[CommitGroup(log, nc, None, 0, None, None) for log, nc in groups])
    else:
        arr = commit_groups(groups)
    v, w = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib.rsv_decommit_sizes(arr, len(groups), log_blowup, n_queries, ctypes.byref(v), ctypes.byref(w)), "rsv_decommit_sizes")
    return v.value, w.value


def composition_log_size(lp: int, lq: int) -> int:
    """rsv_composition_log_size: L3 = max(lp + 2, lq + 3) - 1, the log size of tree 3's eight columns.  Host arithmetic."""
    out = ctypes.c_uint32(0)
    _check(lib.rsv_composition_log_size(lp, lq, ctypes.byref(out)), "rsv_composition_log_size")
    return int(out.value)


def fri_sizes(lp: int, lq: int, log_blowup: int, log_last: int) -> dict:
    """rsv_fri_sizes: {"sizes": the quotient columns' LDE log sizes, descending, "n_inner", "quot_words", "layer_words",
    "last_words": words per proof of d_quot, d_layers, d_last_poly} for the recursion circuit's shape.  Host arithmetic."""
    sizes = np.zeros(3, np.uint32)
    ns, ni = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    q, lw, last = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    as_p = lambda a: a.ctypes.data_as(_u32p)  # noqa: E731
    _check(lib.rsv_fri_sizes(lp, lq, log_blowup, log_last, as_p(sizes), as_p(ns), as_p(ni), ctypes.byref(q), ctypes.byref(lw), ctypes.byref(last)), "rsv_fri_sizes")
    return {"sizes": [int(v) for v in sizes[:int(ns[0])]], "n_inner": int(ni[0]), "quot_words": q.value, "layer_words": lw.value,
            "last_words": last.value}


def fri_open_sizes(sizes, log_blowup: int, log_last: int, n_queries: int):
    """rsv_fri_open_sizes: (values_cap in QM31 values, witness_cap in nodes) per (proof, tree) of rsv_fri_open_dev's outputs;
    sizes the quotient columns' LDE log sizes, descending.  Host arithmetic."""
    sz = _u32(list(sizes))
    v, w = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib.rsv_fri_open_sizes(sz.ctypes.data_as(_u32p), len(sz), log_blowup, log_last, n_queries, ctypes.byref(v), ctypes.byref(w)),
           "rsv_fri_open_sizes")
    return v.value, w.value


def fri_cap_sizes(sizes, log_blowup: int, log_last: int, sub_log: int, n: int = 1):
    """rsv_fri_cap_sizes: (cap_words, tree_words): the words of d_caps for n proofs and per layer tree the words before it; layer
    l (1 .. max(top - sub_log, 0)) of tree t is uint32[n, 2^l, 8] at tree_words[t] + n * 8 * (2^l - 2).  Host arithmetic."""
    sz = _u32(list(sizes))
    words = ctypes.c_size_t()
    trees = (ctypes.c_size_t * 32)()
    _check(lib.rsv_fri_cap_sizes(sz.ctypes.data_as(_u32p), len(sz), log_blowup, log_last, sub_log, n, ctypes.byref(words), trees), "rsv_fri_cap_sizes")
    return words.value, [int(trees[t]) for t in range(int(sz[0]) - log_last - log_blowup)]


def proof_bytes_bound(log_last: int, n_layers: int, counts) -> int:
    """rsv_proof_bytes: the length in bytes of a serialised proof with the given counts, 8 + 2 n_layers of them: values of
    trees 0-3, witness nodes of trees 0-3, then per layer tree its fri_witness values and hash_witness nodes.  With the
    capacities of the buffers it is the bound a d_blob is sized with, with a proof's own counts its length.  Host arithmetic."""
    c = _u32(list(counts))
    if len(c) != 8 + 2 * n_layers:
        raise ValueError(f"proof_bytes_bound: {len(c)} counts for {n_layers} layer trees")
    out = ctypes.c_size_t()
    _check(lib.rsv_proof_bytes(log_last, n_layers, c.ctypes.data_as(_u32p), ctypes.byref(out)), "rsv_proof_bytes")
    return out.value


def proof_list(d_items, stride: int, d_count, count_stride: int, cap: int, items_at: int = 0, count_at: int = 0) -> ProofList:
    """An rsv_proof_list over tensors of 32-bit words: the items from word items_at of d_items with `stride` words per proof,
    the counts from word count_at of d_count with count_stride words per proof."""
    return ProofList(d_items.data_ptr() + 4 * items_at, stride, d_count.data_ptr() + 4 * count_at, count_stride, cap)


def witness_decommit_sizes(program, log_blowup: int, n_queries: int):
    """The capacities of Context.witness_decommit's outputs: ([values_cap of tree 0, 1, 2], witness_cap)."""
    lp, lq = program.trace_sizes()
    sizes = [decommit_sizes([(lp, a), (lq, b)], log_blowup, n_queries) for a, b in ((10, 40), (12, 48), (8, 8))]
    return [v for v, _ in sizes], sizes[0][1]


def fri_paths(proofs: Sequence[bytes], cfg, n_queries: int, max_log: int, n_inner: int, inputs=STANDARD_INPUTS, device: int = 0):
    """per-query pair paths of the FRI trees.  Returns (sib uint32[n,1+n_inner,nq,max_log,8],
    cols uint32[n,1+n_inner,nq,3,8], accept, reason)."""
    blob, offsets = pack(proofs)
    n = len(proofs)
    sib = np.zeros((n, 1 + n_inner, n_queries, max_log, 8), np.uint32)
    cols = np.zeros((n, 1 + n_inner, n_queries, 3, 8), np.uint32)
    accept = np.zeros(n, np.uint8)
    reason = np.zeros(n, np.uint8)
    pi = make_inputs(inputs)
    _check(lib.rsv_fri_paths(blob.ctypes.data_as(_u8p), offsets.ctypes.data_as(_u64p), n, prepare_cfg(cfg, n).ref(), pi, len(list(inputs)), n_queries,
                             max_log, n_inner, sib.ctypes.data_as(_u32p), cols.ctypes.data_as(_u32p),
                             accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), device), "rsv_fri_paths")
    return sib, cols, accept, reason


class HostArena:
    """rsv_host_alloc: pinned host memory the caller reads its proofs into, back to back; `buf` is a numpy uint8 view of it.
    pack(proofs) copies a list of proofs in and returns the HostBatch over the copies (what a caller that deserialises
    straight into the arena would hold)."""

    def __init__(self, nbytes: int):
        h = ctypes.c_void_p()
        _check(lib.rsv_host_alloc(nbytes, ctypes.byref(h)), "rsv_host_alloc")
        self._h = h
        self.nbytes = nbytes
        self.buf = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(h.value))

    def pack(self, proofs) -> "HostBatch":
        views, at = [], 0
        for p in proofs:
            a = np.frombuffer(p, dtype=np.uint8) if not isinstance(p, np.ndarray) else p
            if at + a.size > self.nbytes:
                raise ValueError("arena too small")
            self.buf[at:at + a.size] = a
            views.append(self.buf[at:at + a.size])
            at += a.size
        return HostBatch(views)

    def close(self):
        if self._h:
            self.buf = None
            lib.rsv_host_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBatch:
    """The argument of rsv_verify_batch_host as a Rust caller holds it (a Vec of serialized proofs = pointers + lengths): built
    once from a list of bytes / numpy uint8 buffers, which it keeps alive."""

    def __init__(self, proofs):
        self.keep = [np.frombuffer(p, dtype=np.uint8) if not isinstance(p, np.ndarray) else p for p in proofs]
        self.n = len(self.keep)
        self.ptrs = (ctypes.c_void_p * max(self.n, 1))(*[k.ctypes.data for k in self.keep])
        self.lens = np.array([k.size for k in self.keep], dtype=np.uint64)
        self.bytes = int(self.lens.sum())


class Context:
    """One HIP stream + reusable HBM workspace on one device (rsv_ctx).  Operates on torch tensors that
    already live on that device; nothing is copied through the host.

    Stream ordering: the context enqueues on its own non-blocking streams.  Every method that reads or writes
    caller tensors first makes the context wait for torch's CURRENT stream (rsv_ctx_wait_stream), so tensors
    produced by torch kernels / copies immediately before the call are complete when the verifier reads them, and
    output buffers freshly allocated or zeroed by torch are not overwritten early.  Results are ordered for torch
    by `synchronize()` (host blocks) or `release_to_torch()` (torch's current stream waits, host does not)."""

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p()
        _check(lib.rsv_ctx_create(device, ctypes.byref(h)), "rsv_ctx_create")
        self._h = h
        self.device = device
        self._live = []
        self._dependents = []  # weak references to the Exchange objects created on this context

    def close(self):
        if self._h:
            for ref in self._dependents:  # an exchange enqueues on this context's stream: it goes first (rsv.h)
                x = ref()
                if x is not None:
                    x.close()
            self._dependents = []
            lib.rsv_ctx_destroy(self._h)  # waits for the context's streams
            self._h = None
            self._live = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib.rsv_ctx_synchronize(self._h), "rsv_ctx_synchronize")
        self._live = []

    def set_option(self, name: str, value) -> None:
        """A tuning / diagnostic knob of this context (rsv_ctx_set_option; names in OPTIONS)."""
        _set_option(self._h, name, value)

    def _keep(self, pc, cfg):
        """A per-proof configuration index uploaded INSIDE a call (cfg was a list, not a PreparedCfg the caller holds)
        lives in a torch tensor that the call's first kernel reads later, on this context's stream.  Were it to die with
        the call, torch's caching allocator could hand its memory to the next allocation on torch's stream, which is not
        ordered behind the context's.  So the context holds it: until synchronize() / close(), or — when many calls are
        queued without one — until torch's current stream has been made to wait for the context (release_to_torch), after
        which a reuse of the block is ordered behind every kernel that read it.  (A PreparedCfg the caller made is the
        caller's to keep alive until the work is ordered, like the blob.)"""
        if pc is cfg:
            return
        self._live.append(pc)
        if len(self._live) > 16:
            self.release_to_torch()
            self._live = self._live[-1:]  # the newest belongs to the call that is about to be enqueued

    @property
    def stream(self) -> int:
        return lib.rsv_ctx_stream(self._h) or 0

    def _torch_stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def acquire_from_torch(self):
        """Work enqueued so far on torch's current stream happens before what this context enqueues next."""
        _check(lib.rsv_ctx_wait_stream(self._h, self._torch_stream()), "rsv_ctx_wait_stream")

    def release_to_torch(self):
        """torch's current stream waits for everything this context has enqueued so far (no host block)."""
        _check(lib.rsv_stream_wait_ctx(self._h, self._torch_stream()), "rsv_stream_wait_ctx")

    def prepare_cfg(self, cfg, n: int) -> PreparedCfg:
        """Stage a configuration set for repeated use (the per-proof index of a mixed batch goes to HBM once)."""
        def to_dev(a):
            import torch
            return torch.from_numpy(a).to(torch.device("cuda", self.device))
        return prepare_cfg(cfg, n, to_dev)

    def poseidon2_permute(self, d_in, d_out, d_bad=None):
        n = d_in.numel() // 16
        self.acquire_from_torch()
        _check(lib.rsv_poseidon2_permute_dev(self._h, d_in.data_ptr(), d_out.data_ptr(), n,
                                             d_bad.data_ptr() if d_bad is not None else None), "rsv_poseidon2_permute_dev")

    def poseidon2_emulated(self, d_left, d_right, d_swap, d_rows, d_bad=None):
        """d_left / d_right: (n, 8) u32; d_swap: None or (n,) u8; d_rows: (n, 416, 4) u32 (rsv_poseidon2_emulated_dev)."""
        n = d_left.numel() // 8
        self.acquire_from_torch()
        _check(lib.rsv_poseidon2_emulated_dev(self._h, d_left.data_ptr(), d_right.data_ptr(),
                                              d_swap.data_ptr() if d_swap is not None else None, d_rows.data_ptr(), n,
                                              d_bad.data_ptr() if d_bad is not None else None), "rsv_poseidon2_emulated_dev")

    def verify_batch(self, d_blob, d_offsets, n: int, d_accept, d_reason=None, cfg=None, inputs=STANDARD_INPUTS, d_inputs=None, n_inputs: int = 0):
        """rsv_verify_batch_dev with the inputs the batch shares; with d_inputs (a device tensor of [n, n_inputs, 5] uint32
        records idx, value[4]: every proof its own, what Context.circuit_inputs writes) rsv_verify_batch_inputs_dev."""
        pc = self.prepare_cfg(cfg, n)
        self.acquire_from_torch()
        self._keep(pc, cfg)
        if d_inputs is not None:
            _check(lib.rsv_verify_batch_inputs_dev(self._h, d_blob.data_ptr(), d_offsets.data_ptr(), n, pc.ref(), d_inputs.data_ptr(), n_inputs,
                                                   d_accept.data_ptr(), d_reason.data_ptr() if d_reason is not None else None),
                   "rsv_verify_batch_inputs_dev")
            return
        pi = make_inputs(inputs)
        _check(lib.rsv_verify_batch_dev(self._h, d_blob.data_ptr(), d_offsets.data_ptr(), n, pc.ref(), pi, len(list(inputs)),
                                        d_accept.data_ptr(), d_reason.data_ptr() if d_reason is not None else None),
               "rsv_verify_batch_dev")

    def trace_paths(self, d_blob, d_offsets, n: int, n_queries: int, max_log: int, d_sib, d_pos, d_accept,
                    d_reason=None, cfg=None, inputs=STANDARD_INPUTS):
        pi = make_inputs(inputs)
        pc = self.prepare_cfg(cfg, n)
        self.acquire_from_torch()
        self._keep(pc, cfg)
        _check(lib.rsv_trace_paths_dev(self._h, d_blob.data_ptr(), d_offsets.data_ptr(), n, pc.ref(), pi, len(list(inputs)),
                                       n_queries, max_log, d_sib.data_ptr(), d_pos.data_ptr(), d_accept.data_ptr(),
                                       d_reason.data_ptr() if d_reason is not None else None), "rsv_trace_paths_dev")

    def verify_batch_host(self, proofs, cfg, inputs=STANDARD_INPUTS):
        """Proofs in host memory, one buffer each (bytes / numpy uint8 arrays, or a HostBatch that holds the pointer table of
        such a list already): gather, upload and verify overlap (rsv_verify_batch_host).  Returns (accept, reason) numpy arrays."""
        hb = proofs if isinstance(proofs, HostBatch) else HostBatch(proofs)
        n = hb.n
        accept = np.zeros(n, np.uint8)
        reason = np.zeros(n, np.uint8)
        pi = make_inputs(inputs)
        pc = prepare_cfg(cfg, n)  # host residency: the library uploads the per-proof index chunk by chunk
        _check(lib.rsv_verify_batch_host(self._h, hb.ptrs, hb.lens.ctypes.data_as(_u64p), n, pc.ref(), pi, len(list(inputs)),
                                         accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p)), "rsv_verify_batch_host")
        return accept, reason

    def verify_hints(self, d_blob, d_offsets, n: int, d_accept, d_reason=None, cfg=None, inputs=STANDARD_INPUTS, shape=(0, 0, 0),
                     d_transcript=None, d_trace_sib=None, d_trace_pos=None, d_trace_cols=None, d_fri_sib=None,
                     d_fri_cols=None, d_fri_folded=None, d_query_values=None, d_flow=None, d_flow_swap=None, d_flow_count=None,
                     d_accept_bitmap=None, d_accept_count=None, d_inputs=None, n_inputs: int = 0):
        """One verifying pass that also fills whichever hint outputs are given (rsv_verify_hints_dev; with d_inputs, as
        verify_batch takes them, rsv_verify_hints_inputs_dev).  shape = (n_queries, max_log, n_inner), needed for the path outputs."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        ho = HintsOut(int(shape[0]), int(shape[1]), int(shape[2]), ptr(d_transcript), ptr(d_trace_sib), ptr(d_trace_pos),
                      ptr(d_trace_cols), ptr(d_fri_sib), ptr(d_fri_cols), ptr(d_fri_folded), ptr(d_query_values),
                      ptr(d_flow), ptr(d_flow_swap), ptr(d_flow_count), int(d_flow.shape[1]) if d_flow is not None else 0,
                      ptr(d_accept_bitmap), ptr(d_accept_count))
        pc = self.prepare_cfg(cfg, n)
        self.acquire_from_torch()
        self._keep(pc, cfg)
        if d_inputs is not None:
            _check(lib.rsv_verify_hints_inputs_dev(self._h, d_blob.data_ptr(), d_offsets.data_ptr(), n, pc.ref(), d_inputs.data_ptr(), n_inputs,
                                                   ctypes.byref(ho), d_accept.data_ptr(), ptr(d_reason)), "rsv_verify_hints_inputs_dev")
            return
        pi = make_inputs(inputs)
        _check(lib.rsv_verify_hints_dev(self._h, d_blob.data_ptr(), d_offsets.data_ptr(), n, pc.ref(), pi, len(list(inputs)),
                                        ctypes.byref(ho), d_accept.data_ptr(), ptr(d_reason)), "rsv_verify_hints_dev")

    def witness(self, program: WitnessProgram, d_blob, d_offsets, n: int, d_variables, d_accept, d_reason=None, inputs=STANDARD_INPUTS,
                d_flow=None, d_flow_swap=None, d_inputs=None):
        """rsv_witness_eval_dev: d_variables uint32[n, n_vars, 4] in HBM (optionally the PoseidonFlow: d_flow uint32[n, flow_count,
        32], d_flow_swap uint8[n, flow_count]); enqueued on the context's streams.  d_inputs: int32[n, n_own, 5], every
        proof's own records behind the shared `inputs` (rsv_witness_eval_inputs_dev, for a program built with n_fixed)."""
        pi = make_inputs(inputs)
        pc = self.prepare_cfg(program.cfg(), n)
        self.acquire_from_torch()
        self._keep(pc, None)
        if d_inputs is not None:
            _own_records(d_inputs, n, "Context.witness")
            _check(lib.rsv_witness_eval_inputs_dev(self._h, program._h, d_blob.data_ptr(), d_offsets.data_ptr(), n, pc.ref(), pi, len(list(inputs)),
                                                   d_inputs.data_ptr(), int(d_inputs.shape[1]), d_variables.data_ptr(),
                                                   d_flow.data_ptr() if d_flow is not None else None,
                                                   d_flow_swap.data_ptr() if d_flow_swap is not None else None, d_accept.data_ptr(),
                                                   d_reason.data_ptr() if d_reason is not None else None), "rsv_witness_eval_inputs_dev")
            return
        _check(lib.rsv_witness_eval_dev(self._h, program._h, d_blob.data_ptr(), d_offsets.data_ptr(), n, pc.ref(), pi, len(list(inputs)),
                                        d_variables.data_ptr(), d_flow.data_ptr() if d_flow is not None else None,
                                        d_flow_swap.data_ptr() if d_flow_swap is not None else None, d_accept.data_ptr(),
                                        d_reason.data_ptr() if d_reason is not None else None),
               "rsv_witness_eval_dev")

    def witness_trace(self, program: WitnessProgram, d_variables, d_accept, n: int, d_plonk=None, d_poseidon=None, d_ops=None, d_flow=None,
                      d_flow_swap=None):
        """rsv_witness_trace_dev on what Context.witness wrote: d_plonk uint32[n, 12, 2^lp], d_poseidon uint32[n, 48, 2^lq],
        d_ops uint32[n, n_witness_ops] (any may be None); enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.acquire_from_torch()
        _check(lib.rsv_witness_trace_dev(self._h, program._h, ptr(d_variables), ptr(d_flow), ptr(d_flow_swap), d_accept.data_ptr(), n,
                                         ptr(d_plonk), ptr(d_poseidon), ptr(d_ops)), "rsv_witness_trace_dev")

    def circuit_check(self, program: WitnessProgram, d_variables, n: int, d_ok, d_bad_row):
        """rsv_circuit_check_dev: the reference's check_arithmetics over n witnesses (d_variables in the context's
        witness_layout); d_ok uint8[n] is cleared where a row fails (a proof with 0 on entry is skipped), d_bad_row
        uint32[n] = the smallest failing row or 0xffffffff; enqueued on the context's stream."""
        self.acquire_from_torch()
        _check(lib.rsv_circuit_check_dev(self._h, program._h, d_variables.data_ptr(), n, d_ok.data_ptr(), d_bad_row.data_ptr()),
               "rsv_circuit_check_dev")

    def circuit_flow(self, program: WitnessProgram, d_variables, n: int, d_flow, d_flow_swap, d_ok, d_bad_flow):
        """rsv_circuit_flow_dev: the reference's check_poseidon_invocations, and the flow: d_flow uint32[n, n_flow, 32]
        (in: the halves without a wire; out: every word) and d_flow_swap uint8[n, n_flow]; d_ok and d_bad_flow as
        circuit_check's; enqueued on the context's stream."""
        self.acquire_from_torch()
        _check(lib.rsv_circuit_flow_dev(self._h, program._h, d_variables.data_ptr(), n, d_flow.data_ptr(), d_flow_swap.data_ptr(),
                                        d_ok.data_ptr(), d_bad_flow.data_ptr()), "rsv_circuit_flow_dev")

    def public_input_sum(self, d_inputs, n: int, n_inputs: int, d_z_alpha, d_sum, d_bad=None):
        """rsv_public_input_sum_dev, the statement sum alone: d_inputs [n, n_inputs, 5] records (None with no inputs),
        d_z_alpha uint32[n, 8] = z | alpha, d_sum uint32[n, 4] = sum_k 1 / (value_k + (idx_k mod P) alpha - z), d_bad uint8[n]
        (optional): 1 where a word is not below P; enqueued on the context's stream."""
        self.acquire_from_torch()
        _check(lib.rsv_public_input_sum_dev(self._h, d_inputs.data_ptr() if d_inputs is not None else None, n, n_inputs, d_z_alpha.data_ptr(),
                                            d_sum.data_ptr(), d_bad.data_ptr() if d_bad is not None else None), "rsv_public_input_sum_dev")

    def statement_digest(self, d_inputs, n_groups: int, copies: int, n_own: int, d_stmt, d_bad=None):
        """rsv_statement_digest_dev, the digest of the statements a recursion step verifies: d_inputs [n_groups * copies,
        n_own, 5] records, d_stmt [n_groups, 8, 5] records (idx 4 + k, value (digest[k], 0, 0, 0)) — hash_m31_columns_get_rate
        of the copies * n_own value words of a group, the form verify_batch(d_inputs=) and the next level's call take;
        d_bad uint8[n_groups] (optional): 1 where a value is not an M31 below P; enqueued on the context's stream (the option
        statement_row_max: 1 + the largest n_groups hashed with 16 threads per group)."""
        self.acquire_from_torch()
        ptr = lambda t: t.data_ptr() if t is not None else None
        _check(lib.rsv_statement_digest_dev(self._h, ptr(d_inputs), n_groups, copies, n_own, ptr(d_stmt), ptr(d_bad)), "rsv_statement_digest_dev")

    def circuit_inputs(self, program: WitnessProgram, d_variables, n: int, d_inputs):
        """rsv_circuit_inputs_dev: the statement of each witness, d_inputs [n, program.num_input, 5] records (k,
        variables[k]) for k = 1 .. num_input, from d_variables (in the context's witness_layout); enqueued on the context's
        stream."""
        self.acquire_from_torch()
        _check(lib.rsv_circuit_inputs_dev(self._h, program._h, d_variables.data_ptr(), n, d_inputs.data_ptr()), "rsv_circuit_inputs_dev")

    def circuit_eval(self, program: WitnessProgram, d_inputs, n: int, d_variables, d_flow, d_flow_swap, d_ok, d_bad_input):
        """rsv_circuit_eval_dev: n witnesses of a Circuit made with hints from d_inputs uint32[n, n_inputs, 4] (None with
        no inputs): d_variables (in the context's witness_layout), d_flow uint32[n, n_flow, 32] (in: the halves with neither
        a wire nor a link) and d_flow_swap uint8[n, n_flow] are written for every witness with d_ok != 0; d_ok is cleared
        where an input word is not below P, d_bad_input uint32[n] = the smallest such slot or 0xffffffff; enqueued on the
        context's stream (the option circuit_eval_form: "auto", "per_level", "walk")."""
        self.acquire_from_torch()
        _check(lib.rsv_circuit_eval_dev(self._h, program._h, d_inputs.data_ptr() if d_inputs is not None else None, n, d_variables.data_ptr(),
                                        d_flow.data_ptr(), d_flow_swap.data_ptr(), d_ok.data_ptr(), d_bad_input.data_ptr()),
               "rsv_circuit_eval_dev")

    def witness_groups(self, program: WitnessProgram, d_blob, d_offsets, n_groups: int, d_variables, d_accept, d_member_accept,
                       d_member_reason=None, inputs=STANDARD_INPUTS, d_flow=None, d_flow_swap=None, d_inputs=None):
        """rsv_witness_eval_groups_dev: the batch holds n_groups * copies proofs, copy c of group g's circuit verifies proof
        g * copies + c.  d_variables uint32[n_groups, n_vars, 4], d_accept uint8[n_groups], d_member_accept (and
        d_member_reason) uint8[n_groups * copies]; optionally d_flow uint32[n_groups, copies, flow_count, 32] and d_flow_swap
        uint8[n_groups, copies, flow_count]; enqueued on the context's streams.  d_inputs: int32[n_groups * copies, n_own, 5],
        every member's own records behind the shared `inputs` (rsv_witness_eval_groups_inputs_dev)."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        pi = make_inputs(inputs)
        pc = self.prepare_cfg(program.cfg(), n_groups * program.shape.copies)
        self.acquire_from_torch()
        self._keep(pc, None)
        if d_inputs is not None:
            _own_records(d_inputs, n_groups * program.shape.copies, "Context.witness_groups")
            _check(lib.rsv_witness_eval_groups_inputs_dev(self._h, program._h, d_blob.data_ptr(), d_offsets.data_ptr(), n_groups, pc.ref(), pi,
                                                          len(list(inputs)), d_inputs.data_ptr(), int(d_inputs.shape[1]), d_variables.data_ptr(),
                                                          ptr(d_flow), ptr(d_flow_swap), d_accept.data_ptr(), ptr(d_member_accept),
                                                          ptr(d_member_reason)), "rsv_witness_eval_groups_inputs_dev")
            return
        _check(lib.rsv_witness_eval_groups_dev(self._h, program._h, d_blob.data_ptr(), d_offsets.data_ptr(), n_groups, pc.ref(), pi,
                                               len(list(inputs)), d_variables.data_ptr(), ptr(d_flow), ptr(d_flow_swap), d_accept.data_ptr(),
                                               ptr(d_member_accept), ptr(d_member_reason)), "rsv_witness_eval_groups_dev")

    def witness_trace_groups(self, program: WitnessProgram, d_variables, d_accept, n_groups: int, d_plonk=None, d_poseidon=None, d_ops=None,
                             d_flow=None, d_flow_swap=None):
        """rsv_witness_trace_groups_dev on what Context.witness_groups wrote: one set of columns per group, shapes as
        witness_trace's with n = n_groups; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.acquire_from_torch()
        _check(lib.rsv_witness_trace_groups_dev(self._h, program._h, ptr(d_variables), ptr(d_flow), ptr(d_flow_swap), d_accept.data_ptr(),
                                                n_groups, ptr(d_plonk), ptr(d_poseidon), ptr(d_ops)), "rsv_witness_trace_groups_dev")

    def witness_interaction(self, program: WitnessProgram, d_plonk, d_poseidon, d_accept, d_lookup, n: int, d_int_plonk, d_int_poseidon, d_sums,
                            d_ok=None):
        """rsv_witness_interaction_dev on what Context.witness_trace wrote and d_lookup uint32[n, 8] (z, alpha): d_int_plonk
        uint32[n, 8, 2^lp], d_int_poseidon uint32[n, 8, 2^lq], d_sums uint32[n, 2, 4], d_ok uint8[n] (may be None); enqueued on
        the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.acquire_from_torch()
        _check(lib.rsv_witness_interaction_dev(self._h, program._h, ptr(d_plonk), ptr(d_poseidon), ptr(d_accept), ptr(d_lookup), n,
                                               ptr(d_int_plonk), ptr(d_int_poseidon), ptr(d_sums), ptr(d_ok)), "rsv_witness_interaction_dev")

    def commit_tree(self, groups, n: int, log_blowup: int, d_roots, d_mask=None, d_cap=None):
        """rsv_commit_tree_dev: groups as commit_groups() takes them (dicts of torch tensors), d_roots uint32[n, 8], d_mask
        uint8[n] (may be None); with d_cap uint32[n, 2^(log_blowup + 1), 8], rsv_commit_tree_cap_dev; enqueued on the
        context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        arr = commit_groups(groups)
        self.acquire_from_torch()
        if d_cap is None:
            _check(lib.rsv_commit_tree_dev(self._h, arr, len(groups), n, log_blowup, ptr(d_mask), ptr(d_roots)), "rsv_commit_tree_dev")
        else:
            _check(lib.rsv_commit_tree_cap_dev(self._h, arr, len(groups), n, log_blowup, ptr(d_mask), ptr(d_roots), ptr(d_cap)),
                   "rsv_commit_tree_cap_dev")

    def decommit_tree(self, groups, n: int, log_blowup: int, d_queries, n_queries: int, d_values, d_n_values, d_witness, d_n_witness,
                      d_mask=None, cap_mode: int = CAP_NONE, d_cap=None):
        """rsv_decommit_tree_dev: the opening of the tree commit_tree commits at d_queries uint32[n, n_queries]: d_values
        uint32[n, values_cap], d_n_values uint32[n], d_witness uint32[n, witness_cap, 8], d_n_witness uint32[n] (capacities:
        decommit_sizes); cap_mode CAP_NONE / CAP_WRITE / CAP_READ with d_cap uint32[n, 2^(log_blowup + 1), 8]; enqueued on
        the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        arr = commit_groups(groups)
        self.acquire_from_torch()
        _check(lib.rsv_decommit_tree_dev(self._h, arr, len(groups), n, log_blowup, ptr(d_mask), ptr(d_queries), n_queries, cap_mode,
                                         ptr(d_cap), ptr(d_values), ptr(d_n_values), ptr(d_witness), ptr(d_n_witness)),
               "rsv_decommit_tree_dev")

    def witness_commit(self, program: WitnessProgram, d_plonk, d_poseidon, d_ops, d_accept, n: int, log_blowup: int, d_roots, d_draws,
                       d_int_plonk, d_int_poseidon, d_sums, d_channel=None, d_ok=None, d_caps=None):
        """rsv_witness_commit_dev on what Context.witness_trace wrote: d_roots uint32[n, 3, 8], d_draws uint32[n, 12],
        d_int_plonk uint32[n, 8, 2^lp], d_int_poseidon uint32[n, 8, 2^lq], d_sums uint32[n, 2, 4], d_channel uint32[n, 16] and
        d_ok uint8[n] (may be None); with d_caps uint32[n, 3, 2^(log_blowup + 1), 8], rsv_witness_commit_caps_dev; enqueued on
        the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.acquire_from_torch()
        lead = (self._h, program._h, ptr(d_plonk), ptr(d_poseidon), ptr(d_ops), ptr(d_accept), n, log_blowup, ptr(d_roots), ptr(d_draws),
                ptr(d_int_plonk), ptr(d_int_poseidon), ptr(d_sums), ptr(d_channel), ptr(d_ok))
        if d_caps is None:
            _check(lib.rsv_witness_commit_dev(*lead), "rsv_witness_commit_dev")
        else:
            _check(lib.rsv_witness_commit_caps_dev(*lead, ptr(d_caps)), "rsv_witness_commit_caps_dev")

    def witness_decommit(self, program: WitnessProgram, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, n: int,
                         log_blowup: int, d_queries, n_queries: int, d_values, d_n_values, d_witness, d_n_witness, d_ok=None, d_caps=None):
        """rsv_witness_decommit_dev on what Context.witness_commit left: the openings of trees 0, 1 and 2 at d_queries
        uint32[n, n_queries]: d_values uint32[n, v0 + v1 + v2], d_n_values uint32[n, 3], d_witness uint32[n, 3, w, 8],
        d_n_witness uint32[n, 3] (capacities: witness_decommit_sizes); d_caps as Context.witness_commit wrote them, or None;
        enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.acquire_from_torch()
        _check(lib.rsv_witness_decommit_dev(self._h, program._h, ptr(d_plonk), ptr(d_poseidon), ptr(d_ops), ptr(d_int_plonk),
                                            ptr(d_int_poseidon), ptr(d_accept), ptr(d_ok), n, log_blowup, ptr(d_queries), n_queries,
                                            ptr(d_caps), ptr(d_values), ptr(d_n_values), ptr(d_witness), ptr(d_n_witness)),
               "rsv_witness_decommit_dev")

    def sample_tree(self, groups, n: int, d_points, n_points: int, d_samples, d_mask=None, source: int = SAMPLE_COLUMNS):
        """rsv_sample_tree_dev: the columns of the tree commit_tree commits (source SAMPLE_COLUMNS: d_cols holds evaluations;
        SAMPLE_COEFFS: what a commitment wrote to d_coeffs) at d_points uint32[n, n_points, 8] (x then y): d_samples
        uint32[n, n_points, sum n_cols, 4]; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        arr = commit_groups(groups)
        self.acquire_from_torch()
        _check(lib.rsv_sample_tree_dev(self._h, arr, len(groups), n, ptr(d_mask), source, ptr(d_points), n_points, ptr(d_samples)),
               "rsv_sample_tree_dev")

    def witness_sample(self, program: WitnessProgram, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, n: int, d_oods,
                       d_samples, d_ok=None):
        """rsv_witness_sample_dev on what Context.witness_commit left: sampled_values[0..2] of the next proof at d_oods
        uint32[n, 8], d_samples uint32[n, 134, 4] in the proof's own order; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.acquire_from_torch()
        _check(lib.rsv_witness_sample_dev(self._h, program._h, ptr(d_plonk), ptr(d_poseidon), ptr(d_ops), ptr(d_int_plonk),
                                          ptr(d_int_poseidon), ptr(d_accept), ptr(d_ok), n, ptr(d_oods), ptr(d_samples)),
               "rsv_witness_sample_dev")

    def composition(self, lp: int, lq: int, plonk, poseidon, d_sums, d_draws, n: int, d_comp, d_comp_coeffs=None, d_mask=None):
        """rsv_composition_dev: plonk and poseidon are (preprocessed, trace, interaction) triples of tensors, uint32[n, cols,
        2^log] each, or [1, cols, 2^log] / [cols, 2^log] for a set every proof shares (proof stride 0); d_sums uint32[n, 2, 4],
        d_draws uint32[n, 12]; d_comp and d_comp_coeffs (may be None) uint32[n, 8, 2^L3]; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        cols = []
        for t in tuple(plonk) + tuple(poseidon):
            shared = t is None or t.dim() != 3 or (t.shape[0] == 1 and n > 1)
            cols += [ptr(t), 0 if shared else t.shape[1] * t.shape[2]]
        self.acquire_from_torch()
        _check(lib.rsv_composition_dev(self._h, lp, lq, *cols, ptr(d_sums), ptr(d_draws), ptr(d_mask), n, ptr(d_comp), ptr(d_comp_coeffs)),
               "rsv_composition_dev")

    def witness_tree3(self, program: WitnessProgram, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, n: int,
                      log_blowup: int, d_sums, d_draws, d_channel, d_comp, d_root3, d_oods, d_samples3, d_ok=None, d_cap3=None):
        """rsv_witness_tree3_dev on what Context.witness_commit left (d_sums, d_draws, d_channel uint32[n, 16], updated): d_comp
        uint32[n, 8, 2^L3], d_root3 uint32[n, 8], d_cap3 uint32[n, 2^(log_blowup + 1), 8] (may be None), d_oods uint32[n, 8] as
        Context.witness_sample takes it, d_samples3 uint32[n, 8, 4]; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.acquire_from_torch()
        _check(lib.rsv_witness_tree3_dev(self._h, program._h, ptr(d_plonk), ptr(d_poseidon), ptr(d_ops), ptr(d_int_plonk),
                                         ptr(d_int_poseidon), ptr(d_accept), ptr(d_ok), n, log_blowup, ptr(d_sums), ptr(d_draws),
                                         ptr(d_channel), ptr(d_comp), ptr(d_root3), ptr(d_cap3), ptr(d_oods), ptr(d_samples3)),
               "rsv_witness_tree3_dev")

    def fri_quotients(self, groups, group_points, n: int, log_blowup: int, d_points, n_points: int, d_samples, d_after, d_quot, d_mask=None,
                      source: int = SAMPLE_COLUMNS):
        """rsv_fri_quotients_dev: groups as commit_groups() takes them; group_points per group a list over the points of
        (col_lo, col_hi) pairs, or None where a point applies to none of the group's columns; d_points uint32[n, n_points, 8],
        d_samples uint32[n, n_points, sum n_cols, 4] as Context.sample_tree writes them, d_after uint32[n, 4]; d_quot per proof
        the quotient columns in descending size, each uint32[4, 2^(log_size + log_blowup)]; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        arr = commit_groups(groups)
        gp = (FriGroupPoints * max(len(groups), 1))()
        for i, pts in enumerate(group_points):
            for k, r in enumerate(pts):
                if r is not None:
                    gp[i].col_lo[k], gp[i].col_hi[k] = r
        self.acquire_from_torch()
        _check(lib.rsv_fri_quotients_dev(self._h, arr, gp, len(groups), n, log_blowup, ptr(d_mask), source, ptr(d_points), n_points,
                                         ptr(d_samples), ptr(d_after), ptr(d_quot)), "rsv_fri_quotients_dev")

    def fri_commit(self, d_quot, sizes, log_blowup: int, log_last: int, n: int, d_channel, d_roots, d_alphas, d_layers, d_last_poly,
                   d_low_degree, d_mask=None, sub_log: int = 0, d_caps=None, tail_log: int = 0):
        """rsv_fri_commit_dev: d_quot as Context.fri_quotients wrote it, sizes its columns' LDE log sizes (descending);
        d_channel uint32[n, 16] (updated), d_roots uint32[n, 1 + n_inner, 8], d_alphas uint32[n, 1 + n_inner, 4], d_layers the
        inner layers per proof (may be None when there is none), d_last_poly uint32[n, 2^log_last, 4], d_low_degree uint8[n];
        with sub_log or d_caps uint32[cap_words] (fri_cap_sizes), rsv_fri_commit_cap_dev; with tail_log (1 .. 10),
        rsv_fri_commit_tail_dev: the same outputs through fewer launches; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        sz = _u32(list(sizes))
        self.acquire_from_torch()
        lead = (self._h, ptr(d_quot), sz.ctypes.data_as(_u32p), len(sz), log_blowup, log_last, n, ptr(d_mask), ptr(d_channel), ptr(d_roots),
                ptr(d_alphas), ptr(d_layers), ptr(d_last_poly), ptr(d_low_degree))
        if tail_log:
            _check(lib.rsv_fri_commit_tail_dev(*lead, sub_log, ptr(d_caps), tail_log), "rsv_fri_commit_tail_dev")
        elif d_caps is None and not sub_log:
            _check(lib.rsv_fri_commit_dev(*lead), "rsv_fri_commit_dev")
        else:
            _check(lib.rsv_fri_commit_cap_dev(*lead, sub_log, ptr(d_caps)), "rsv_fri_commit_cap_dev")

    def witness_fri(self, program: WitnessProgram, d_plonk, d_poseidon, d_ops, d_int_plonk, d_int_poseidon, d_accept, n: int,
                    log_blowup: int, log_last: int, d_comp, d_oods, d_samples, d_samples3, d_channel, d_after, d_quot, d_roots, d_alphas,
                    d_layers, d_last_poly, d_low_degree, d_ok=None, sub_log: int = 0, d_caps=None, tail_log: int = 0):
        """rsv_witness_fri_dev on what Context.witness_tree3 and Context.witness_sample left (d_comp, d_oods, d_samples3,
        d_samples uint32[n, 134, 4], d_channel uint32[n, 16], updated): d_after uint32[n, 4], d_quot uint32[n, quot_words],
        d_layers uint32[n, layer_words] (fri_sizes), and the outputs of Context.fri_commit; with sub_log or d_caps,
        rsv_witness_fri_caps_dev; with tail_log, rsv_witness_fri_tail_dev; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.acquire_from_torch()
        lead = (self._h, program._h, ptr(d_plonk), ptr(d_poseidon), ptr(d_ops), ptr(d_int_plonk), ptr(d_int_poseidon), ptr(d_accept), ptr(d_ok), n,
                log_blowup, log_last, ptr(d_comp), ptr(d_oods), ptr(d_samples), ptr(d_samples3), ptr(d_channel), ptr(d_after), ptr(d_quot),
                ptr(d_roots), ptr(d_alphas), ptr(d_layers), ptr(d_last_poly), ptr(d_low_degree))
        if tail_log:
            _check(lib.rsv_witness_fri_tail_dev(*lead, sub_log, ptr(d_caps), tail_log), "rsv_witness_fri_tail_dev")
        elif d_caps is None and not sub_log:
            _check(lib.rsv_witness_fri_dev(*lead), "rsv_witness_fri_dev")
        else:
            _check(lib.rsv_witness_fri_caps_dev(*lead, sub_log, ptr(d_caps)), "rsv_witness_fri_caps_dev")

    def pow_grind(self, pow_bits: int, n: int, d_ok, d_channel, d_nonce, start: int = 0, max_tries: int = 0):
        """rsv_pow_grind_dev: the smallest nonce >= start (of max_tries candidates; 0: 2^(pow_bits + 6)) whose mix into
        d_channel uint32[n, 16] leaves pow_bits low zero bits in digest word 0: d_nonce uint32[n, 2] (low word first), the
        channel updated; d_ok uint8[n] is the mask and is cleared where the search is exhausted; enqueued on the context's
        stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.acquire_from_torch()
        _check(lib.rsv_pow_grind_dev(self._h, pow_bits, start, max_tries, n, ptr(d_ok), ptr(d_channel), ptr(d_nonce)), "rsv_pow_grind_dev")

    def draw_queries(self, n: int, n_queries: int, log_size: int, log_size_low: int, d_channel, d_queries, d_queries_low=None, d_mask=None):
        """rsv_draw_queries_dev: ceil(n_queries / 8) draws from d_channel uint32[n, 16] (updated): d_queries uint32[n,
        n_queries] the positions of log_size bits in draw order, d_queries_low (may be None) the same >> (log_size -
        log_size_low); d_mask uint8[n] (may be None); enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.acquire_from_torch()
        _check(lib.rsv_draw_queries_dev(self._h, n, ptr(d_mask), n_queries, log_size, log_size_low, ptr(d_channel), ptr(d_queries),
                                        ptr(d_queries_low)), "rsv_draw_queries_dev")

    def fri_open(self, d_quot, d_layers, sizes, log_blowup: int, log_last: int, n: int, d_queries, n_queries: int, d_fri_witness,
                 d_n_fri_witness, d_hash_witness, d_n_hash_witness, d_mask=None, sub_log: int = 0, d_caps=None):
        """rsv_fri_open_dev on what Context.fri_commit took and left (d_quot, sizes, d_layers; d_layers may be None when there
        is no inner layer) at d_queries uint32[n, n_queries] (positions of sizes[0] bits): d_fri_witness uint32[n, T,
        values_cap, 4], d_n_fri_witness uint32[n, T], d_hash_witness uint32[n, T, witness_cap, 8], d_n_hash_witness uint32[n,
        T] (T = 1 + n_inner; capacities: fri_open_sizes); with sub_log or d_caps (what Context.fri_commit left under the same
        sub_log), rsv_fri_open_cap_dev; enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        sz = _u32(list(sizes))
        self.acquire_from_torch()
        lead = (self._h, ptr(d_quot), ptr(d_layers), sz.ctypes.data_as(_u32p), len(sz), log_blowup, log_last, n, ptr(d_mask), ptr(d_queries),
                n_queries, ptr(d_fri_witness), ptr(d_n_fri_witness), ptr(d_hash_witness), ptr(d_n_hash_witness))
        if d_caps is None and not sub_log:
            _check(lib.rsv_fri_open_dev(*lead), "rsv_fri_open_dev")
        else:
            _check(lib.rsv_fri_open_cap_dev(*lead, sub_log, ptr(d_caps)), "rsv_fri_open_cap_dev")

    def proof_pack(self, parts: ProofParts, n: int, d_blob, d_offsets, d_mask=None, blob_cap=None):
        """rsv_proof_pack_dev: the n proofs `parts` (a ProofParts; its lists from proof_list) points at, serialised into d_blob
        uint8 (None: offsets only) with d_offsets int64[n + 1]; a proof whose end lies beyond blob_cap bytes (default: all of
        d_blob) is not written; d_mask uint8[n] (may be None); enqueued on the context's stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        if blob_cap is None:
            blob_cap = d_blob.numel() * d_blob.element_size() if d_blob is not None else 0
        self.acquire_from_torch()
        _check(lib.rsv_proof_pack_dev(self._h, ctypes.byref(parts), n, ptr(d_mask), ptr(d_blob), blob_cap, ptr(d_offsets)), "rsv_proof_pack_dev")

    def accept_bitmap(self, d_accept, n: int, d_bitmap, d_count=None):
        self.acquire_from_torch()
        _check(lib.rsv_accept_bitmap_dev(self._h, d_accept.data_ptr(), n, d_bitmap.data_ptr(),
                                         d_count.data_ptr() if d_count is not None else None), "rsv_accept_bitmap_dev")

    def last_stage_times(self) -> dict:
        names = (ctypes.c_char_p * 16)()
        ms = (ctypes.c_float * 16)()
        k = lib.rsv_last_stage_times(self._h, names, ms, 16)
        if k < 0:
            raise RsvError(k, "rsv_last_stage_times")
        return {names[i].decode(): float(ms[i]) for i in range(k)}


def shard_range(n_total: int, rank: int, world: int):
    """rsv_shard_range: the contiguous [lo, hi) of rank `rank` (the rule sharding.shard_range restates in Python)."""
    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
    lib.rsv_shard_range(n_total, rank, world, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def shard_plan(lens, world: int):
    """rsv_shard_plan: contiguous cuts balanced by bytes.  lens: the job's proof lengths.  Returns (lo, hi), `world` entries each."""
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    lo, hi = (ctypes.c_size_t * world)(), (ctypes.c_size_t * world)()
    _check(lib.rsv_shard_plan(ln.ctypes.data_as(_u64p), len(ln), world, lo, hi), "rsv_shard_plan")
    return list(lo), list(hi)


def cfg_check(cfg: "PcsConfig") -> bool:
    """rsv_cfg_check: is the configuration inside the library's shape limits (include/rsv.h: RSV_MAX_*)?"""
    return lib.rsv_cfg_check(ctypes.byref(cfg)) == 0


class MultiContext:
    """rsv_multi: ONE process drives several contexts (one per entry of `devices`; a device may repeat), one host thread
    per context per call; the job's verdicts, bitmap and count are assembled on the host (no collective)."""

    def __init__(self, devices: Sequence[int]):
        arr = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        _check(lib.rsv_multi_create(arr, len(devices), ctypes.byref(h)), "rsv_multi_create")
        self._h = h
        self.devices = list(devices)

    def close(self):
        if self._h:
            lib.rsv_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(lib.rsv_multi_size(self._h))

    def set_option(self, name: str, value) -> None:
        for r in range(len(self)):
            _set_option(ctypes.c_void_p(lib.rsv_multi_ctx(self._h, r)), name, value)

    def verify_batch_host(self, proofs, cfg, inputs=STANDARD_INPUTS):
        """The whole job in host memory (bytes / numpy buffers or a HostBatch).  Returns (accept, reason, bitmap, count)."""
        hb = proofs if isinstance(proofs, HostBatch) else HostBatch(proofs)
        n = hb.n
        accept, reason = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        bitmap = np.zeros(max(1, (n + 31) // 32), np.uint32)
        count = ctypes.c_uint64()
        pi = make_inputs(inputs)
        pc = prepare_cfg(cfg, n)
        _check(lib.rsv_multi_verify_batch_host(self._h, hb.ptrs, hb.lens.ctypes.data_as(_u64p), n, pc.ref(), pi, len(list(inputs)),
                                               accept.ctypes.data_as(_u8p), reason.ctypes.data_as(_u8p), bitmap.ctypes.data_as(_u32p),
                                               ctypes.byref(count)), "rsv_multi_verify_batch_host")
        return accept, reason, bitmap[: (n + 31) // 32], int(count.value)

    def verify_batch_dev(self, shards, cfg_table: Sequence[PcsConfig], inputs=STANDARD_INPUTS):
        """shards: one dict per context with torch tensors on that context's device: d_blob, d_offsets, n, and optionally
        d_cfg_of / d_accept / d_reason.  The caller has synchronised whatever produced them (the call waits for nothing
        of torch's).  Returns (bitmap uint32[ceil(sum n / 32)], count)."""
        if len(shards) != len(self):
            raise ValueError("one shard per context")
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        arr = (Shard * len(shards))(*[Shard(ptr(s["d_blob"]), ptr(s["d_offsets"]), int(s["n"]), ptr(s.get("d_cfg_of")),
                                            ptr(s.get("d_accept")), ptr(s.get("d_reason"))) for s in shards])
        n_total = sum(int(s["n"]) for s in shards)
        bitmap = np.zeros(max(1, (n_total + 31) // 32), np.uint32)
        count = ctypes.c_uint64()
        pi = make_inputs(inputs)
        pc = PreparedCfg(list(cfg_table))
        _check(lib.rsv_multi_verify_batch_dev(self._h, arr, len(shards), pc.ref(), pi, len(list(inputs)), bitmap.ctypes.data_as(_u32p),
                                              ctypes.byref(count)), "rsv_multi_verify_batch_dev")
        return bitmap[: (n_total + 31) // 32], int(count.value)


def exchange_available() -> bool:
    return bool(lib.rsv_exchange_available())


def exchange_unique_id() -> bytes:
    buf = (ctypes.c_uint8 * EXCHANGE_ID_BYTES)()
    _check(lib.rsv_exchange_unique_id(buf), "rsv_exchange_unique_id")
    return bytes(buf)


def exchange_assemble(n_total: int, world: int, gathered: np.ndarray, plan=None):
    """rsv_exchange_assemble[_plan]: gathered [world][slice_words] (host) -> (accept bytes, contiguous bitmap) of the job.
    plan = (lo, hi) of every rank for a job cut by rsv_shard_plan (or by the caller); None: rsv_shard_range's cuts."""
    g = np.ascontiguousarray(gathered, dtype=np.uint32)
    accept = np.zeros(max(n_total, 1), np.uint8)
    bitmap = np.zeros(max(1, (n_total + 31) // 32), np.uint32)
    if plan is None:
        _check(lib.rsv_exchange_assemble(n_total, world, g.ctypes.data_as(_u32p), accept.ctypes.data_as(_u8p), bitmap.ctypes.data_as(_u32p)),
               "rsv_exchange_assemble")
    else:
        lo, hi = (ctypes.c_size_t * world)(*plan[0]), (ctypes.c_size_t * world)(*plan[1])
        _check(lib.rsv_exchange_assemble_plan(world, lo, hi, g.ctypes.data_as(_u32p), accept.ctypes.data_as(_u8p), bitmap.ctypes.data_as(_u32p)),
               "rsv_exchange_assemble_plan")
    return accept[:n_total], bitmap[: (n_total + 31) // 32]


class Exchange:
    """rsv_exchange: the one-process-per-GPU collective step over RCCL, driven through the C-ABI (no torch.distributed on
    the data path).  `uid` = exchange_unique_id() of rank 0, distributed by the caller.  Collective constructor."""

    def __init__(self, ctx: "Context", uid: bytes, rank: int, world: int, n_total: int, plan=None):
        """plan = (lo, hi) of every rank (rsv_shard_plan's cuts, or the caller's): rsv_exchange_create_plan; None: the job is
        cut by rsv_shard_range.  Close the exchange before its context (rsv.h)."""
        buf = (ctypes.c_uint8 * EXCHANGE_ID_BYTES).from_buffer_copy(uid)
        h = ctypes.c_void_p()
        if plan is None:
            _check(lib.rsv_exchange_create(ctx._h, buf, rank, world, n_total, ctypes.byref(h)), "rsv_exchange_create")
        else:
            lo_a, hi_a = (ctypes.c_size_t * world)(*plan[0]), (ctypes.c_size_t * world)(*plan[1])
            _check(lib.rsv_exchange_create_plan(ctx._h, buf, rank, world, lo_a, hi_a, ctypes.byref(h)), "rsv_exchange_create_plan")
        self._h, self.ctx, self.rank, self.world, self.n_total = h, ctx, rank, world, n_total
        ctx._dependents.append(weakref.ref(self))
        lo, hi, sw = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib.rsv_exchange_layout(h, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(sw)), "rsv_exchange_layout")
        self.lo, self.hi, self.slice_words = lo.value, hi.value, sw.value

    def run(self, d_local, d_gathered, d_count=None):
        _check(lib.rsv_exchange_run(self._h, d_local.data_ptr(), d_gathered.data_ptr(), d_count.data_ptr() if d_count is not None else None),
               "rsv_exchange_run")

    def close(self):
        if self._h:
            lib.rsv_exchange_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


from . import witness_program  # noqa: E402,F401  (the witness program container)
from .chain import Chain  # noqa: E402,F401  (the next-proof chain's buffers and stages as one object)
