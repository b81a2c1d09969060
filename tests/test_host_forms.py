"""The refusals of the host-pointer entry points, without a device: ONE table, a row per entry point and misuse — each null
pointer, each size limit, each configuration beyond RSV_MAX_*, each out-of-range word, `flow` without `flow_swap`, a hints
output whose pair is missing, a device index that does not exist — and a well-formed call of every form, which without a
device ends at RSV_E_DEVICE (no CPU fallback).  Each row carries its status code.

Provenance: the codes are those of a build of commit b9e5200, the parent of the change that moved these entry points onto
one staging path (csrc/host_stage.inc): the table was run against that build first (the binding loaded with its library,
every row's status compared) and only then against the new code; where a row and that build disagreed the build's code was
taken (one row: rsv_verify_batch_inputs, n_pi without pi in an empty batch, RSV_E_NULL).  It passes unchanged on both."""
import ctypes

import numpy as np
import pytest

from tests import user_circuit_ref as U

OK, NULL, SIZE, DEVICE, CAP, RANGE = 0, -1, -2, -3, -4, -5
P = 0x7FFFFFFF
NO_DEVICE = 99  # an index no machine has


class Env:
    """Buffers the rows share.  Every array is large enough for the n a row passes with it; the rows that pass a huge n are
    refused before anything is read."""

    def __init__(self, rsv):
        self.rsv, self.lib = rsv, rsv.lib
        self.w = np.zeros(4096, np.uint32)              # canonical words
        self.bad = np.full(4096, P, np.uint32)          # every word out of range
        self.b = np.zeros(4096, np.uint8)
        self.offs = np.array([0, 64, 128], np.uint64)
        self.params = np.zeros(26, np.uint32)
        self.params[:2] = 4                             # the two log sizes of rsv_oods_eval's params26
        self.ncols = np.ones(32, np.uint32)
        self.cfg = rsv.PreparedCfg([rsv.PcsConfig(20, 5, 8, 16)])
        self.pi = (rsv.PublicInput * 4)()
        self.bad_pi = (rsv.PublicInput * 4)()
        self.bad_pi[1].value[2] = P
        b = U.build("S1")
        self.circuit = rsv.Circuit(b.gates, b.flow_wires, b.n_vars, b.num_input, b.witness_ops)  # a caller's circuit: no instructions
        self.prog = self.circuit._h

    def u32(self, a=None):
        return (self.w if a is None else a).ctypes.data_as(self.rsv._u32p)

    def u8(self):
        return self.b.ctypes.data_as(self.rsv._u8p)

    def o(self):
        return self.offs.ctypes.data_as(self.rsv._u64p)

    def cfgs(self, *cfgs, n_cfgs=None, cfgs_null=False):
        """An rsv_cfg_set of the given (pow_bits, log_blowup, log_last, n_queries) tuples, with the count or the array falsified."""
        pc = self.rsv.PreparedCfg([self.rsv.PcsConfig(*c) for c in cfgs])
        if n_cfgs is not None:
            pc.struct.n_cfgs = n_cfgs
        if cfgs_null:
            pc.struct.cfgs = None
        self.keep = pc
        return pc.ref()

    def hints(self, **fields):
        h = self.rsv.HintsOut()
        for k, v in fields.items():
            setattr(h, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        self.keep_h = h
        return ctypes.byref(h)


GOOD = (20, 5, 8, 16)
BEYOND = {"n_queries 129": (20, 5, 8, 129), "n_queries 0": (20, 5, 8, 0), "log_blowup 17": (20, 17, 8, 16), "log_blowup 0": (20, 0, 8, 16),
          "log_last 17": (20, 5, 17, 16), "pow_bits 31": (31, 5, 8, 16)}


def _batch_rows(name, call):
    """The rows every batch form shares: call(e, blob, offsets, n, cfg, accept, device) -> status."""
    rows = [
        (name, "null blob", NULL, lambda e: call(e, None, e.o(), 2, e.cfg.ref(), e.u8(), 0)),
        (name, "null offsets", NULL, lambda e: call(e, e.u8(), None, 2, e.cfg.ref(), e.u8(), 0)),
        (name, "null cfg", NULL, lambda e: call(e, e.u8(), e.o(), 2, None, e.u8(), 0)),
        (name, "null cfgs array", NULL, lambda e: call(e, e.u8(), e.o(), 2, e.cfgs(GOOD, cfgs_null=True), e.u8(), 0)),
        (name, "n_cfgs 0", SIZE, lambda e: call(e, e.u8(), e.o(), 2, e.cfgs(GOOD, n_cfgs=0), e.u8(), 0)),
        (name, "n_cfgs 17", SIZE, lambda e: call(e, e.u8(), e.o(), 2, e.cfgs(GOOD, n_cfgs=17), e.u8(), 0)),
        (name, "empty batch, null cfg", NULL, lambda e: call(e, None, None, 0, None, None, 0)),
        (name, "second configuration beyond", SIZE, lambda e: call(e, e.u8(), e.o(), 2, e.cfgs(GOOD, (20, 5, 8, 129)), e.u8(), 0)),
        (name, "no such device", DEVICE, lambda e: call(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), NO_DEVICE)),
        (name, "empty batch, no such device", DEVICE, lambda e: call(e, None, None, 0, e.cfg.ref(), None, NO_DEVICE)),
        (name, "well-formed, no device", DEVICE, lambda e: call(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0)),
    ]
    for what, c in BEYOND.items():
        rows.append((name, what, SIZE, lambda e, c=c: call(e, e.u8(), e.o(), 2, e.cfgs(c), e.u8(), 0)))
    return rows


def _witness_rows(name, call, outputs):
    """The rows the witness chain's host forms share: call(e, prog, blob, offsets, n, accept, device, **outputs set to NULL)."""
    rows = [
        (name, "null program", NULL, lambda e: call(e, None, e.u8(), e.o(), 2, e.u8(), 0)),
        (name, "null blob", NULL, lambda e: call(e, e.prog, None, e.o(), 2, e.u8(), 0)),
        (name, "null offsets", NULL, lambda e: call(e, e.prog, e.u8(), None, 2, e.u8(), 0)),
        (name, "null accept", NULL, lambda e: call(e, e.prog, e.u8(), e.o(), 2, None, 0)),
        (name, "a caller's circuit", SIZE, lambda e: call(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0)),
        (name, "a caller's circuit, no such device", SIZE, lambda e: call(e, e.prog, e.u8(), e.o(), 2, e.u8(), NO_DEVICE)),
    ]
    for out in outputs:
        rows.append((name, "null " + out, NULL, lambda e, out=out: call(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0, **{out: None})))
    return rows


def _verify_batch(e, blob, offs, n, cfg, acc, dev, pi=None, n_pi=0):
    return e.lib.rsv_verify_batch(blob, offs, n, cfg, pi, n_pi, acc, None, dev)


def _verify_batch_inputs(e, blob, offs, n, cfg, acc, dev, pi=None, n_pi=0):
    return e.lib.rsv_verify_batch_inputs(blob, offs, n, cfg, pi, n_pi, acc, None, dev)


def _verify_hints(e, blob, offs, n, cfg, acc, dev, out="default", pi=None, n_pi=0):
    return e.lib.rsv_verify_hints(blob, offs, n, cfg, pi, n_pi, e.hints(d_transcript=e.w) if out == "default" else out, acc, None, dev)


def _trace_paths(e, blob, offs, n, cfg, acc, dev, sib="w", pos="w", nq=16, max_log=20):
    return e.lib.rsv_trace_paths(blob, offs, n, cfg, None, 0, nq, max_log, e.u32() if sib else None, e.u32() if pos else None, acc, None, dev)


def _fri_paths(e, blob, offs, n, cfg, acc, dev, sib="w", cols="w"):
    return e.lib.rsv_fri_paths(blob, offs, n, cfg, None, 0, 16, 20, 5, e.u32() if sib else None, e.u32() if cols else None, acc, None, dev)


def _transcript_batch(e, blob, offs, n, cfg, acc, dev, out="w"):
    return e.lib.rsv_transcript_batch(blob, offs, n, cfg, e.u32() if out else None, dev)


def _witness_eval(e, prog, blob, offs, n, acc, dev, variables="w", flow=None, flow_swap=None):
    return e.lib.rsv_witness_eval(prog, blob, offs, n, e.cfg.ref(), None, 0, e.u32() if variables else None, e.u32() if flow else None,
                                  e.u8() if flow_swap else None, acc, None, dev)


def _witness_eval_inputs(e, prog, blob, offs, n, acc, dev, variables="w", flow=None, flow_swap=None, fixed=None, n_fixed=0, own=None, n_own=0):
    return e.lib.rsv_witness_eval_inputs(prog, blob, offs, n, e.cfg.ref(), fixed, n_fixed, own, n_own, e.u32() if variables else None,
                                         e.u32() if flow else None, e.u8() if flow_swap else None, acc, None, dev)


def _witness_trace(e, prog, blob, offs, n, acc, dev):
    return e.lib.rsv_witness_trace(prog, blob, offs, n, e.cfg.ref(), None, 0, e.u32(), e.u32(), e.u32(), acc, None, dev)


def _witness_interaction(e, prog, blob, offs, n, acc, dev, lookup="w", int_plonk="w", int_poseidon="w", sums="w"):
    p = lambda x: e.u32() if x else None
    return e.lib.rsv_witness_interaction(prog, blob, offs, n, e.cfg.ref(), None, 0, p(lookup), p(int_plonk), p(int_poseidon), p(sums), None,
                                         acc, None, dev)


def _witness_commit(e, prog, blob, offs, n, acc, dev, roots="w", draws="w", sums="w", log_blowup=1):
    p = lambda x: e.u32() if x else None
    return e.lib.rsv_witness_commit(prog, blob, offs, n, e.cfg.ref(), None, 0, log_blowup, p(roots), p(draws), p(sums), None, acc, None, dev)


BIG = 1 << 40  # beyond every n limit; the rows that pass it are refused before a buffer is read

ROWS = [
    # ---- the eleven probes
    ("rsv_poseidon2_permute", "null in", NULL, lambda e: e.lib.rsv_poseidon2_permute(None, e.u32(), 1, 0)),
    ("rsv_poseidon2_permute", "null out", NULL, lambda e: e.lib.rsv_poseidon2_permute(e.u32(), None, 1, 0)),
    ("rsv_poseidon2_permute", "n beyond 2^28", SIZE, lambda e: e.lib.rsv_poseidon2_permute(e.u32(), e.u32(), (1 << 28) + 1, 0)),
    ("rsv_poseidon2_permute", "no such device", DEVICE, lambda e: e.lib.rsv_poseidon2_permute(e.u32(), e.u32(), 1, NO_DEVICE)),
    ("rsv_poseidon2_permute", "n 0, no such device", DEVICE, lambda e: e.lib.rsv_poseidon2_permute(None, None, 0, NO_DEVICE)),
    ("rsv_poseidon2_permute", "well-formed, no device", DEVICE, lambda e: e.lib.rsv_poseidon2_permute(e.u32(), e.u32(), 1, 0)),
    ("rsv_poseidon2_half_permute", "null left", NULL, lambda e: e.lib.rsv_poseidon2_half_permute(None, e.u32(), None, e.u32(), e.u32(), 1, 0)),
    ("rsv_poseidon2_half_permute", "null right", NULL, lambda e: e.lib.rsv_poseidon2_half_permute(e.u32(), None, None, e.u32(), e.u32(), 1, 0)),
    ("rsv_poseidon2_half_permute", "n beyond 2^28", SIZE, lambda e: e.lib.rsv_poseidon2_half_permute(e.u32(), e.u32(), None, e.u32(), e.u32(), (1 << 28) + 1, 0)),
    ("rsv_poseidon2_half_permute", "no such device", DEVICE, lambda e: e.lib.rsv_poseidon2_half_permute(e.u32(), e.u32(), None, e.u32(), e.u32(), 1, NO_DEVICE)),
    ("rsv_poseidon2_half_permute", "no outputs, no device", DEVICE, lambda e: e.lib.rsv_poseidon2_half_permute(e.u32(), e.u32(), None, None, None, 1, 0)),
    ("rsv_poseidon2_emulated", "null left", NULL, lambda e: e.lib.rsv_poseidon2_emulated(None, e.u32(), None, e.u32(), 1, 0)),
    ("rsv_poseidon2_emulated", "null right", NULL, lambda e: e.lib.rsv_poseidon2_emulated(e.u32(), None, None, e.u32(), 1, 0)),
    ("rsv_poseidon2_emulated", "null rows", NULL, lambda e: e.lib.rsv_poseidon2_emulated(e.u32(), e.u32(), None, None, 1, 0)),
    ("rsv_poseidon2_emulated", "n beyond 2^22", SIZE, lambda e: e.lib.rsv_poseidon2_emulated(e.u32(), e.u32(), None, e.u32(), (1 << 22) + 1, 0)),
    ("rsv_poseidon2_emulated", "no such device", DEVICE, lambda e: e.lib.rsv_poseidon2_emulated(e.u32(), e.u32(), None, e.u32(), 1, NO_DEVICE)),
    ("rsv_poseidon2_emulated", "well-formed, no device", DEVICE, lambda e: e.lib.rsv_poseidon2_emulated(e.u32(), e.u32(), e.u8(), e.u32(), 1, 0)),
    ("rsv_merkle_hash_node", "null out", NULL, lambda e: e.lib.rsv_merkle_hash_node(e.u32(), e.u32(), None, 0, None, 1, 0)),
    ("rsv_merkle_hash_node", "left without right", NULL, lambda e: e.lib.rsv_merkle_hash_node(e.u32(), None, None, 0, e.u32(), 1, 0)),
    ("rsv_merkle_hash_node", "right without left", NULL, lambda e: e.lib.rsv_merkle_hash_node(None, e.u32(), None, 0, e.u32(), 1, 0)),
    ("rsv_merkle_hash_node", "n_cols without cols", NULL, lambda e: e.lib.rsv_merkle_hash_node(e.u32(), e.u32(), None, 3, e.u32(), 1, 0)),
    ("rsv_merkle_hash_node", "neither children nor columns", SIZE, lambda e: e.lib.rsv_merkle_hash_node(None, None, None, 0, e.u32(), 1, 0)),
    ("rsv_merkle_hash_node", "n beyond 2^26", SIZE, lambda e: e.lib.rsv_merkle_hash_node(e.u32(), e.u32(), None, 0, e.u32(), (1 << 26) + 1, 0)),
    ("rsv_merkle_hash_node", "n_cols beyond 4096", SIZE, lambda e: e.lib.rsv_merkle_hash_node(None, None, e.u32(), 4097, e.u32(), 1, 0)),
    ("rsv_merkle_hash_node", "no such device", DEVICE, lambda e: e.lib.rsv_merkle_hash_node(e.u32(), e.u32(), None, 0, e.u32(), 1, NO_DEVICE)),
    ("rsv_merkle_hash_node", "well-formed, no device", DEVICE, lambda e: e.lib.rsv_merkle_hash_node(e.u32(), e.u32(), e.u32(), 3, e.u32(), 1, 0)),
    ("rsv_merkle_path_root", "null query", NULL, lambda e: e.lib.rsv_merkle_path_root(None, e.u32(), e.u32(), e.u32(e.ncols), 3, e.u32(), 1, 0)),
    ("rsv_merkle_path_root", "null siblings", NULL, lambda e: e.lib.rsv_merkle_path_root(e.u32(), None, e.u32(), e.u32(e.ncols), 3, e.u32(), 1, 0)),
    ("rsv_merkle_path_root", "null cols", NULL, lambda e: e.lib.rsv_merkle_path_root(e.u32(), e.u32(), None, e.u32(e.ncols), 3, e.u32(), 1, 0)),
    ("rsv_merkle_path_root", "null n_cols_at", NULL, lambda e: e.lib.rsv_merkle_path_root(e.u32(), e.u32(), e.u32(), None, 3, e.u32(), 1, 0)),
    ("rsv_merkle_path_root", "null out", NULL, lambda e: e.lib.rsv_merkle_path_root(e.u32(), e.u32(), e.u32(), e.u32(e.ncols), 3, None, 1, 0)),
    ("rsv_merkle_path_root", "depth 32", SIZE, lambda e: e.lib.rsv_merkle_path_root(e.u32(), e.u32(), e.u32(), e.u32(e.ncols), 32, e.u32(), 1, 0)),
    ("rsv_merkle_path_root", "no column at the leaves", SIZE, lambda e: e.lib.rsv_merkle_path_root(e.u32(), e.u32(), e.u32(), e.u32(), 3, e.u32(), 1, 0)),
    ("rsv_merkle_path_root", "n beyond 2^24", SIZE, lambda e: e.lib.rsv_merkle_path_root(e.u32(), e.u32(), e.u32(), e.u32(e.ncols), 3, e.u32(), (1 << 24) + 1, 0)),
    ("rsv_merkle_path_root", "4097 columns at a level", SIZE,
     lambda e: e.lib.rsv_merkle_path_root(e.u32(), e.u32(), e.u32(), e.u32(np.array([1, 4097, 1, 1], np.uint32)), 3, e.u32(), 1, 0)),
    ("rsv_merkle_path_root", "no such device", DEVICE, lambda e: e.lib.rsv_merkle_path_root(e.u32(), e.u32(), e.u32(), e.u32(e.ncols), 3, e.u32(), 1, NO_DEVICE)),
    ("rsv_merkle_path_root", "depth 0 without siblings, no device", DEVICE, lambda e: e.lib.rsv_merkle_path_root(e.u32(), None, e.u32(), e.u32(e.ncols), 0, e.u32(), 1, 0)),
    ("rsv_field_op", "null a", NULL, lambda e: e.lib.rsv_field_op(0, None, e.u32(), e.u32(), 1, 0)),
    ("rsv_field_op", "null out", NULL, lambda e: e.lib.rsv_field_op(0, e.u32(), e.u32(), None, 1, 0)),
    ("rsv_field_op", "binary op without b", NULL, lambda e: e.lib.rsv_field_op(e.rsv.F_QMUL, e.u32(), None, e.u32(), 1, 0)),
    ("rsv_field_op", "op -1", SIZE, lambda e: e.lib.rsv_field_op(-1, e.u32(), e.u32(), e.u32(), 1, 0)),
    ("rsv_field_op", "op beyond the last", SIZE, lambda e: e.lib.rsv_field_op(e.rsv.F_QPOW + 1, e.u32(), e.u32(), e.u32(), 1, 0)),
    ("rsv_field_op", "n beyond 2^26", SIZE, lambda e: e.lib.rsv_field_op(0, e.u32(), e.u32(), e.u32(), (1 << 26) + 1, 0)),
    ("rsv_field_op", "word of a out of range", RANGE, lambda e: e.lib.rsv_field_op(e.rsv.F_QMUL, e.u32(e.bad), e.u32(), e.u32(), 1, 0)),
    ("rsv_field_op", "word of b out of range", RANGE, lambda e: e.lib.rsv_field_op(e.rsv.F_QMUL, e.u32(), e.u32(e.bad), e.u32(), 1, 0)),
    ("rsv_field_op", "exponent words are not field elements, no device", DEVICE, lambda e: e.lib.rsv_field_op(e.rsv.F_QPOW, e.u32(), e.u32(e.bad), e.u32(), 1, 0)),
    ("rsv_field_op", "no such device", DEVICE, lambda e: e.lib.rsv_field_op(0, e.u32(), e.u32(), e.u32(), 1, NO_DEVICE)),
    ("rsv_domain_points", "null q", NULL, lambda e: e.lib.rsv_domain_points(10, None, e.u32(), 1, 0)),
    ("rsv_domain_points", "null xy", NULL, lambda e: e.lib.rsv_domain_points(10, e.u32(), None, 1, 0)),
    ("rsv_domain_points", "log_size 0", SIZE, lambda e: e.lib.rsv_domain_points(0, e.u32(), e.u32(), 1, 0)),
    ("rsv_domain_points", "log_size beyond RSV_MAX_LOG_SIZE", SIZE, lambda e: e.lib.rsv_domain_points(31, e.u32(), e.u32(), 1, 0)),
    ("rsv_domain_points", "n beyond 2^26", SIZE, lambda e: e.lib.rsv_domain_points(10, e.u32(), e.u32(), (1 << 26) + 1, 0)),
    ("rsv_domain_points", "no such device", DEVICE, lambda e: e.lib.rsv_domain_points(10, e.u32(), e.u32(), 1, NO_DEVICE)),
    ("rsv_domain_points", "well-formed, no device", DEVICE, lambda e: e.lib.rsv_domain_points(10, e.u32(), e.u32(), 1, 0)),
    ("rsv_line_eval", "null coeffs", NULL, lambda e: e.lib.rsv_line_eval(None, 2, e.u32(), e.u32(), 1, 0)),
    ("rsv_line_eval", "null x", NULL, lambda e: e.lib.rsv_line_eval(e.u32(), 2, None, e.u32(), 1, 0)),
    ("rsv_line_eval", "null out", NULL, lambda e: e.lib.rsv_line_eval(e.u32(), 2, e.u32(), None, 1, 0)),
    ("rsv_line_eval", "log_n 17", SIZE, lambda e: e.lib.rsv_line_eval(e.u32(), 17, e.u32(), e.u32(), 1, 0)),
    ("rsv_line_eval", "n beyond 2^26", SIZE, lambda e: e.lib.rsv_line_eval(e.u32(), 2, e.u32(), e.u32(), (1 << 26) + 1, 0)),
    ("rsv_line_eval", "coefficient out of range", RANGE, lambda e: e.lib.rsv_line_eval(e.u32(e.bad), 2, e.u32(), e.u32(), 1, 0)),
    ("rsv_line_eval", "x out of range", RANGE, lambda e: e.lib.rsv_line_eval(e.u32(), 2, e.u32(e.bad), e.u32(), 1, 0)),
    ("rsv_line_eval", "no such device", DEVICE, lambda e: e.lib.rsv_line_eval(e.u32(), 2, e.u32(), e.u32(), 1, NO_DEVICE)),
    ("rsv_last_layer_check", "null coeffs", NULL, lambda e: e.lib.rsv_last_layer_check(None, 2, e.u32(), e.u32(), e.u8(), 1, 0)),
    ("rsv_last_layer_check", "null x", NULL, lambda e: e.lib.rsv_last_layer_check(e.u32(), 2, None, e.u32(), e.u8(), 1, 0)),
    ("rsv_last_layer_check", "null folded", NULL, lambda e: e.lib.rsv_last_layer_check(e.u32(), 2, e.u32(), None, e.u8(), 1, 0)),
    ("rsv_last_layer_check", "null ok", NULL, lambda e: e.lib.rsv_last_layer_check(e.u32(), 2, e.u32(), e.u32(), None, 1, 0)),
    ("rsv_last_layer_check", "log_n 17", SIZE, lambda e: e.lib.rsv_last_layer_check(e.u32(), 17, e.u32(), e.u32(), e.u8(), 1, 0)),
    ("rsv_last_layer_check", "n beyond 2^26", SIZE, lambda e: e.lib.rsv_last_layer_check(e.u32(), 2, e.u32(), e.u32(), e.u8(), (1 << 26) + 1, 0)),
    ("rsv_last_layer_check", "coefficient out of range", RANGE, lambda e: e.lib.rsv_last_layer_check(e.u32(e.bad), 2, e.u32(), e.u32(), e.u8(), 1, 0)),
    ("rsv_last_layer_check", "x out of range", RANGE, lambda e: e.lib.rsv_last_layer_check(e.u32(), 2, e.u32(e.bad), e.u32(), e.u8(), 1, 0)),
    ("rsv_last_layer_check", "folded out of range", RANGE, lambda e: e.lib.rsv_last_layer_check(e.u32(), 2, e.u32(), e.u32(e.bad), e.u8(), 1, 0)),
    ("rsv_last_layer_check", "no such device", DEVICE, lambda e: e.lib.rsv_last_layer_check(e.u32(), 2, e.u32(), e.u32(), e.u8(), 1, NO_DEVICE)),
    ("rsv_oods_eval", "null samples", NULL, lambda e: e.lib.rsv_oods_eval(None, e.u32(e.params), e.u32(), 1, 0)),
    ("rsv_oods_eval", "null params", NULL, lambda e: e.lib.rsv_oods_eval(e.u32(), None, e.u32(), 1, 0)),
    ("rsv_oods_eval", "null out", NULL, lambda e: e.lib.rsv_oods_eval(e.u32(), e.u32(e.params), None, 1, 0)),
    ("rsv_oods_eval", "n beyond 2^20", SIZE, lambda e: e.lib.rsv_oods_eval(e.u32(), e.u32(e.params), e.u32(), (1 << 20) + 1, 0)),
    ("rsv_oods_eval", "sample out of range", RANGE, lambda e: e.lib.rsv_oods_eval(e.u32(e.bad), e.u32(e.params), e.u32(), 1, 0)),
    ("rsv_oods_eval", "log size 0 in params", RANGE, lambda e: e.lib.rsv_oods_eval(e.u32(), e.u32(), e.u32(), 1, 0)),
    ("rsv_oods_eval", "log size 29 in params", RANGE, lambda e: e.lib.rsv_oods_eval(e.u32(), e.u32(np.array([4, 29] + [0] * 24, np.uint32)), e.u32(), 1, 0)),
    ("rsv_oods_eval", "parameter word out of range", RANGE, lambda e: e.lib.rsv_oods_eval(e.u32(), e.u32(np.array([4, 4] + [0] * 23 + [P], np.uint32)), e.u32(), 1, 0)),
    ("rsv_oods_eval", "no such device", DEVICE, lambda e: e.lib.rsv_oods_eval(e.u32(), e.u32(e.params), e.u32(), 1, NO_DEVICE)),
    ("rsv_oods_eval", "well-formed, no device", DEVICE, lambda e: e.lib.rsv_oods_eval(e.u32(), e.u32(e.params), e.u32(), 1, 0)),
    ("rsv_transcript", "null proof", NULL, lambda e: e.lib.rsv_transcript(None, 64, e.u32(), 512, 0)),
    ("rsv_transcript", "null out", NULL, lambda e: e.lib.rsv_transcript(e.u8(), 64, None, 512, 0)),
    ("rsv_transcript", "cap 0", CAP, lambda e: e.lib.rsv_transcript(e.u8(), 64, e.u32(), 0, 0)),
    ("rsv_transcript", "len beyond 2^30", SIZE, lambda e: e.lib.rsv_transcript(e.u8(), (1 << 30) + 1, e.u32(), 512, 0)),
    ("rsv_transcript", "no such device", DEVICE, lambda e: e.lib.rsv_transcript(e.u8(), 64, e.u32(), 512, NO_DEVICE)),
    ("rsv_transcript", "well-formed, no device", DEVICE, lambda e: e.lib.rsv_transcript(e.u8(), 64, e.u32(), 512, 0)),
    # ---- the batch forms
    *_batch_rows("rsv_verify_batch", _verify_batch),
    ("rsv_verify_batch", "null accept", NULL, lambda e: _verify_batch(e, e.u8(), e.o(), 2, e.cfg.ref(), None, 0)),
    ("rsv_verify_batch", "n_pi without pi", NULL, lambda e: _verify_batch(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, None, 3)),
    ("rsv_verify_batch", "n_pi without pi, empty batch", NULL, lambda e: _verify_batch(e, None, None, 0, e.cfg.ref(), None, 0, None, 3)),
    ("rsv_verify_batch", "no n limit of its own, no device", DEVICE, lambda e: _verify_batch(e, e.u8(), e.o(), BIG, e.cfg.ref(), e.u8(), 0)),
    *_batch_rows("rsv_verify_batch_inputs", _verify_batch_inputs),
    ("rsv_verify_batch_inputs", "null accept", NULL, lambda e: _verify_batch_inputs(e, e.u8(), e.o(), 2, e.cfg.ref(), None, 0)),
    ("rsv_verify_batch_inputs", "n_pi without pi", NULL, lambda e: _verify_batch_inputs(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, None, 2)),
    ("rsv_verify_batch_inputs", "n_pi without pi, empty batch", NULL, lambda e: _verify_batch_inputs(e, None, None, 0, e.cfg.ref(), None, 0, None, 2)),
    ("rsv_verify_batch_inputs", "n beyond 2^26", SIZE, lambda e: _verify_batch_inputs(e, e.u8(), e.o(), (1 << 26) + 1, e.cfg.ref(), e.u8(), 0)),
    ("rsv_verify_batch_inputs", "n_pi beyond 4096", SIZE, lambda e: _verify_batch_inputs(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, e.pi, 4097)),
    ("rsv_verify_batch_inputs", "n * n_pi beyond RSV_MAX_INPUT_RECORDS", SIZE, lambda e: _verify_batch_inputs(e, e.u8(), e.o(), 1 << 26, e.cfg.ref(), e.u8(), 0, e.pi, 4096)),
    ("rsv_verify_batch_inputs", "configuration beyond, ahead of the n limit", SIZE, lambda e: _verify_batch_inputs(e, e.u8(), e.o(), BIG, e.cfgs((20, 5, 8, 129)), e.u8(), 0)),
    ("rsv_verify_batch_inputs", "input word out of range", RANGE, lambda e: _verify_batch_inputs(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, e.bad_pi, 2)),
    ("rsv_verify_batch_inputs", "input word out of range, no such device", RANGE, lambda e: _verify_batch_inputs(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), NO_DEVICE, e.bad_pi, 2)),
    *_batch_rows("rsv_verify_hints", _verify_hints),
    ("rsv_verify_hints", "null out", NULL, lambda e: _verify_hints(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, out=None)),
    ("rsv_verify_hints", "null out, empty batch", NULL, lambda e: _verify_hints(e, None, None, 0, e.cfg.ref(), None, 0, out=None)),
    ("rsv_verify_hints", "null accept", NULL, lambda e: _verify_hints(e, e.u8(), e.o(), 2, e.cfg.ref(), None, 0)),
    ("rsv_verify_hints", "n_pi without pi", NULL, lambda e: _verify_hints(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, n_pi=1)),
    ("rsv_verify_hints", "n beyond 2^20", SIZE, lambda e: _verify_hints(e, e.u8(), e.o(), (1 << 20) + 1, e.cfg.ref(), e.u8(), 0)),
    ("rsv_verify_hints", "configuration beyond, ahead of the n limit", SIZE, lambda e: _verify_hints(e, e.u8(), e.o(), BIG, e.cfgs((20, 5, 8, 129)), e.u8(), 0)),
    ("rsv_verify_hints", "flow without flow_swap, no device", DEVICE,
     lambda e: _verify_hints(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, out=e.hints(d_flow=e.w, flow_stride=8))),
    ("rsv_verify_hints", "trace_sib without trace_pos, no device", DEVICE,
     lambda e: _verify_hints(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, out=e.hints(d_trace_sib=e.w, n_queries=16, max_log=20))),
    *_batch_rows("rsv_trace_paths", _trace_paths),
    ("rsv_trace_paths", "sib without pos", NULL, lambda e: _trace_paths(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, pos=None)),
    ("rsv_trace_paths", "pos without sib", NULL, lambda e: _trace_paths(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, sib=None)),
    ("rsv_trace_paths", "n beyond 2^20", SIZE, lambda e: _trace_paths(e, e.u8(), e.o(), (1 << 20) + 1, e.cfg.ref(), e.u8(), 0)),
    ("rsv_trace_paths", "n_queries beyond RSV_MAX_QUERIES, no device", DEVICE, lambda e: _trace_paths(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, nq=129)),
    *_batch_rows("rsv_fri_paths", _fri_paths),
    ("rsv_fri_paths", "sib without cols", NULL, lambda e: _fri_paths(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, cols=None)),
    ("rsv_fri_paths", "cols without sib", NULL, lambda e: _fri_paths(e, e.u8(), e.o(), 2, e.cfg.ref(), e.u8(), 0, sib=None)),
    ("rsv_fri_paths", "n beyond 2^20", SIZE, lambda e: _fri_paths(e, e.u8(), e.o(), (1 << 20) + 1, e.cfg.ref(), e.u8(), 0)),
    *_batch_rows("rsv_transcript_batch", _transcript_batch),
    ("rsv_transcript_batch", "null out", NULL, lambda e: _transcript_batch(e, e.u8(), e.o(), 2, e.cfg.ref(), None, 0, out=None)),
    ("rsv_transcript_batch", "n beyond 2^20", SIZE, lambda e: _transcript_batch(e, e.u8(), e.o(), (1 << 20) + 1, e.cfg.ref(), None, 0)),
    # ---- the witness chain's host forms (a program with instructions needs a device to exist: what is reachable here is
    # ---- every check ahead of "a caller's circuit")
    *_witness_rows("rsv_witness_eval", _witness_eval, ("variables",)),
    ("rsv_witness_eval", "flow without flow_swap", NULL, lambda e: _witness_eval(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0, flow="w")),
    ("rsv_witness_eval", "flow_swap without flow", NULL, lambda e: _witness_eval(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0, flow_swap="b")),
    ("rsv_witness_eval", "a caller's circuit, empty batch", SIZE, lambda e: _witness_eval(e, e.prog, None, None, 0, None, 0, variables=None)),
    ("rsv_witness_eval", "a caller's circuit, ahead of the n limit", SIZE, lambda e: _witness_eval(e, e.prog, e.u8(), e.o(), (1 << 20) + 1, e.u8(), 0)),
    *_witness_rows("rsv_witness_eval_inputs", _witness_eval_inputs, ("variables",)),
    ("rsv_witness_eval_inputs", "flow without flow_swap", NULL, lambda e: _witness_eval_inputs(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0, flow="w")),
    ("rsv_witness_eval_inputs", "flow_swap without flow", NULL, lambda e: _witness_eval_inputs(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0, flow_swap="b")),
    ("rsv_witness_eval_inputs", "a caller's circuit, ahead of the records' checks", SIZE,
     lambda e: _witness_eval_inputs(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0, n_fixed=2, n_own=2)),
    *_witness_rows("rsv_witness_trace", _witness_trace, ()),
    ("rsv_witness_trace", "a caller's circuit, empty batch", SIZE, lambda e: _witness_trace(e, e.prog, None, None, 0, None, 0)),
    *_witness_rows("rsv_witness_interaction", _witness_interaction, ("lookup", "int_plonk", "int_poseidon", "sums")),
    ("rsv_witness_interaction", "a caller's circuit, empty batch", SIZE, lambda e: _witness_interaction(e, e.prog, None, None, 0, None, 0)),
    *_witness_rows("rsv_witness_commit", _witness_commit, ("roots", "draws", "sums")),
    ("rsv_witness_commit", "log_blowup 0", SIZE, lambda e: _witness_commit(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0, log_blowup=0)),
    ("rsv_witness_commit", "log_blowup 17", SIZE, lambda e: _witness_commit(e, e.prog, e.u8(), e.o(), 2, e.u8(), 0, log_blowup=17)),
    ("rsv_witness_commit", "log_blowup 0, empty batch", SIZE, lambda e: _witness_commit(e, e.prog, None, None, 0, None, 0, log_blowup=0)),
]


@pytest.fixture(scope="module")
def env(rsv):
    e = Env(rsv)
    yield e
    e.circuit.close()


def test_the_table_names_every_host_pointer_form():
    names = {r[0] for r in ROWS}
    assert names == {"rsv_poseidon2_permute", "rsv_poseidon2_half_permute", "rsv_poseidon2_emulated", "rsv_merkle_hash_node", "rsv_merkle_path_root",
                     "rsv_field_op", "rsv_domain_points", "rsv_line_eval", "rsv_last_layer_check", "rsv_oods_eval", "rsv_transcript",
                     "rsv_verify_batch", "rsv_verify_batch_inputs", "rsv_verify_hints", "rsv_trace_paths", "rsv_fri_paths", "rsv_transcript_batch",
                     "rsv_witness_eval", "rsv_witness_eval_inputs", "rsv_witness_trace", "rsv_witness_interaction", "rsv_witness_commit"}
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS)  # no row twice


def test_every_refusal_keeps_its_code(env):
    """Every row of the table.  The rows whose misuse is only "there is no device" (device 0, everything else well-formed)
    hold on a machine without one; with a device those calls go through and are the GPU tests' to check."""
    has_device = env.rsv.device_count() > 0
    wrong = []
    for name, misuse, code, call in ROWS:
        if has_device and misuse.endswith("no device"):
            continue
        got = call(env)
        if got != code:
            wrong.append((name, misuse, code, got))
    assert not wrong, wrong
