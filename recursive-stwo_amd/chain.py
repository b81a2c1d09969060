"""Chain: the buffers and stages of "the next proof on the GPU" as one object.

Every stage of the chain up to FRI (Context.witness, witness_trace, witness_commit, witness_decommit, witness_tree3,
witness_sample, witness_fri) takes the same program, trace columns and flags, followed by its own tensors.  A Chain owns those tensors,
allocates each when the stage that writes it first runs, and makes each Context call with the arguments drawn from itself.
The Context methods stay the 1:1 layer over the C-ABI; nothing here reaches past them.  Chain.proofs() puts what the stages
left into the bytes of a PlonkWithPoseidonProof (proof_bytes: plain numpy on the host, the definition of the bytes);
Chain.pack() puts the same bytes into a (blob, offsets) pair on the device (Context.proof_pack), which Chain.witness of the
next level takes as it is.
"""
import numpy as np

from . import (CAP_NONE, CAP_READ, Circuit, ProofParts, composition_log_size, decommit_sizes, fri_cap_sizes, fri_open_sizes, fri_sizes, pack,
               proof_bytes_bound, proof_list, witness_decommit_sizes)

_FLAGS = ("acc", "ok", "low_degree", "member_accept", "member_reason")
_WRITTEN = ("acc", "bad_row", "bad_flow", "bad_input","member_accept", "member_reason", "plonk", "poseidon", "ops", "roots", "draws", "int_plonk", "int_poseidon", "sums", "channel", "ok", "caps", "comp", "root3",
            "oods", "samples3", "cap3", "samples", "after", "quot", "fri_roots", "alphas", "layers", "last_poly", "low_degree", "fri_caps",
            "nonce", "queries", "queries_low", "values", "n_values", "witness_nodes", "n_witness", "values3", "n_values3", "witness3", "n_witness3",
            "fri_witness", "n_fri_witness", "fri_hash_witness", "n_fri_hash_witness")
SAMPLES_PER_COLUMN = ([1] * 50, [1] * 60, [1, 1, 1, 1, 2, 2, 2, 2] * 2, [1] * 8)  # sampled_values of trees 0-3


def _u64(v):
    return np.array([int(v) & 0xFFFFFFFF, int(v) >> 32], np.uint32)


def _vec(items):
    """A bincode Vec of fixed-size items: the u64 count, then the words of items uint32[count, width]."""
    items = np.asarray(items, np.uint32)
    return [_u64(len(items)), items.reshape(-1)]


def proof_bytes(lp, lq, sums, config, commitments, samples, openings, nonce, layers, last_poly, log_last):
    """The serialised PlonkWithPoseidonProof (bincode: little-endian words, u64 length prefixes).
    sums uint32[2, 4]; config (pow_bits, log_blowup, log_last, n_queries); commitments uint32[4, 8]; samples uint32[142, 4],
    tree-major, column-major, sample-minor; openings: per tree 0-3 (queried values uint32[nv], hash witness uint32[nw, 8]);
    nonce uint32[2], low word first; layers: the first layer, then the inner ones, each (fri_witness uint32[nf, 4],
    hash_witness uint32[nh, 8], commitment uint32[8]); last_poly uint32[2^log_last, 4].  Every column_witness is empty."""
    pow_bits, log_blowup, cfg_last, n_queries = config
    out = [np.array([lp, lq], np.uint32), np.asarray(sums, np.uint32).reshape(8), np.array([pow_bits, log_blowup, cfg_last], np.uint32),
           _u64(n_queries)]
    out += _vec(np.asarray(commitments, np.uint32).reshape(4, 8))
    samples, at = np.asarray(samples, np.uint32).reshape(-1, 4), 0
    out.append(_u64(len(SAMPLES_PER_COLUMN)))
    for tree in SAMPLES_PER_COLUMN:
        out.append(_u64(len(tree)))
        for k in tree:
            out += _vec(samples[at:at + k])
            at += k
    assert at == len(samples) and sum(len(x) for x in out) == 895
    out.append(_u64(len(openings)))
    for _, witness in openings:
        out += _vec(np.asarray(witness, np.uint32).reshape(-1, 8)) + [_u64(0)]
    out.append(_u64(len(openings)))
    for values, _ in openings:
        out += _vec(np.asarray(values, np.uint32).reshape(-1, 1))
    out.append(np.asarray(nonce, np.uint32).reshape(2))
    for i, (fri_witness, hash_witness, commitment) in enumerate(layers):
        if i == 1:
            out.append(_u64(len(layers) - 1))
        out += _vec(np.asarray(fri_witness, np.uint32).reshape(-1, 4)) + _vec(np.asarray(hash_witness, np.uint32).reshape(-1, 8))
        out += [_u64(0), np.asarray(commitment, np.uint32).reshape(8)]
    if len(layers) == 1:
        out.append(_u64(0))
    out += _vec(np.asarray(last_poly, np.uint32).reshape(-1, 4)) + [np.array([log_last], np.uint32)]
    return np.concatenate(out).astype("<u4").tobytes()


class Chain:
    """Chain(ctx, program, n, log_blowup): n proofs through witness() -> trace() -> commit() -> decommit() / tree3() ->
    sample() -> fri() -> pow() -> open() / fri_open() -> proofs() or pack().  The tensors are attributes (None until their stage has run): uint32 words as int32, the flags acc,
    ok and low_degree uint8.  Outputs are prefilled with `fill` (the flags ok and low_degree with 7 where fill is not 0), so
    a word a stage leaves unwritten shows.  caps=True also keeps the caps of trees 0-2 (commit) and of tree 3 (tree3);
    fri_sub_log = h (1 .. 8) also keeps the caps of the FRI layer trees (fri), from which fri_open() then rebuilds subtrees
    of at most 2^h leaves only; fri_tail_log = t (1 .. 10) runs fri()'s commit phase in the tail form (the same outputs through
    fewer launches).  aggregate=True: n is the number of GROUPS of program.shape.copies proofs; copy c of group g's circuit
    verifies proof g * copies + c of the batch witness() takes, every tensor and the next proof are per group, and
    member_accept, member_reason [n, copies] hold the members' own verdicts.  With a Circuit as the program the chain
    starts at load() (the caller's witnesses) or evaluate() (the witnesses computed on the device from their free
    inputs) instead of witness(), and there is no aggregation."""

    def __init__(self, ctx, program, n, log_blowup, *, log_last=None, fill=0, caps=False, fri_sub_log=0, fri_tail_log=0, device="cuda:0",
                 aggregate=False):
        self.ctx, self.program, self.n, self.log_blowup, self.log_last = ctx, program, n, log_blowup, log_last
        self.aggregate = aggregate
        if aggregate and isinstance(program, Circuit):
            raise ValueError("Chain: aggregate=True needs a built program, not a Circuit")
        self.fill, self.with_caps, self.fri_sub_log, self.fri_tail_log, self.device = fill, caps, fri_sub_log, fri_tail_log, device
        self.lp, self.lq = program.trace_sizes()
        self.n_ops = len(program.gates()[1])
        self.done = set()
        self.pow_bits = None
        self._blob = self._vars = self._flow = self._swap = None
        self._inputs = self._packed = None
        for name in _WRITTEN:
            setattr(self, name, None)

    def _new(self, *shape, flag=False, fill=None):
        import torch
        fill = self.fill if fill is None else fill
        if flag:
            return torch.full(shape, 7 if fill else 0, dtype=torch.uint8, device=self.device)
        return torch.full(shape, fill - (1 << 32) if fill >> 31 else fill, dtype=torch.int32, device=self.device)

    def _need(self, stage, *before):
        for b in before:
            if b not in self.done:
                raise ValueError(f"Chain.{stage}() needs {b}() first")

    def witness(self, proofs_or_blob, inputs, by_variable=False, *, d_inputs=None):
        """Context.witness on proofs (a list of bytes) or a packed (blob, offsets): numpy arrays, or device tensors (uint8
        and int64[n + 1], what pack() returns), which are used as they are; by_variable: the context's witness_layout
        option is "by_variable".  With aggregate: n * copies proofs, group after group.  d_inputs: a device tensor
        int32[n, n_own, 5] (with aggregate [n * copies, n_own, 5]), every proof's own records behind the shared `inputs` —
        what inputs() of the chain that made the proofs returns, minus the shared records — for a program built with
        n_fixed: the own inputs become this chain's statements."""
        import torch
        if isinstance(self.program, Circuit):
            raise ValueError("Chain.witness() evaluates the recursion circuit: a Circuit's witness comes through load()")
        blob, offsets = pack(proofs_or_blob) if isinstance(proofs_or_blob, list) else proofs_or_blob
        n, wp = self.n, self.program
        if torch.is_tensor(blob):
            self._blob = (blob, offsets)
        else:
            self._blob = (torch.from_numpy(blob.copy()).to(self.device), torch.from_numpy(offsets.astype(np.int64)).to(self.device))
        F = wp.shape.flow_count
        self._vars = self._new(*((wp.n_vars, n, 4) if by_variable else (n, wp.n_vars, 4)), fill=0)
        self.acc = self._new(n, flag=True, fill=0)
        S = wp.stmt_flow  # a hashed program: the records of the statement hash follow the members', [n, S] behind [n (* m), F]
        if self.aggregate:
            m = wp.shape.copies
            if S:
                self._flow, self._swap = self._new(n * (m * F + S), 32, fill=0), self._new(n * (m * F + S), flag=True, fill=0)
            else:
                self._flow, self._swap = self._new(n, m, F, 32, fill=0), self._new(n, m, F, flag=True, fill=0)
            self.member_accept, self.member_reason = self._new(n, m, flag=True, fill=0), self._new(n, m, flag=True, fill=0)
            self.ctx.witness_groups(wp, *self._blob, n, self._vars, self.acc, self.member_accept, self.member_reason, inputs=inputs,
                                    d_flow=self._flow, d_flow_swap=self._swap, d_inputs=d_inputs)
        else:
            if S:
                self._flow, self._swap = self._new(n * (F + S), 32, fill=0), self._new(n * (F + S), flag=True, fill=0)
            else:
                self._flow, self._swap = self._new(n, F, 32, fill=0), self._new(n, F, flag=True, fill=0)
            self.ctx.witness(wp, *self._blob, n, self._vars, self.acc, inputs=inputs, d_flow=self._flow, d_flow_swap=self._swap, d_inputs=d_inputs)
        self._gather_inputs()
        self.done = {"witness"}

    def load(self, variables, flow=None, swap=None, check=True, by_variable=False):
        """The caller's witnesses in the place of witness(): variables uint32[n, n_vars, 4] ([n_vars, n, 4] with
        by_variable: the context's witness_layout option is "by_variable"), flow uint32[n, n_flow, 32] and swap
        uint8[n, n_flow] (None: zeros); numpy arrays, or device tensors, which are used as they are (the flow is written).
        check=True: Context.circuit_check and circuit_flow — acc is 1 where both of the reference's checks pass, bad_row
        and bad_flow [n] hold the first failing row and invocation (all ones: none), and the flow is the one
        circuit_flow made from `variables` and the halves without a wire.  check=False: everything is taken as given
        and acc is ones.  Not with aggregate."""
        import torch
        if self.aggregate:
            raise ValueError("Chain.load() is not for aggregate=True")
        n, wp = self.n, self.program
        if wp.stmt_flow:
            raise ValueError("Chain.load() is not for a hashed program (its flow buffers end in the records of the statement hash): use witness()")
        F = wp.shape.copies * wp.shape.flow_count

        def dev(x, shape, dtype):
            if x is None:
                return torch.zeros(shape, dtype=dtype, device=self.device)
            if not torch.is_tensor(x):
                x = np.ascontiguousarray(x, np.uint8 if dtype == torch.uint8 else np.uint32)
                x = torch.from_numpy(x if dtype == torch.uint8 else x.view(np.int32)).to(self.device)
            if tuple(x.shape) != shape or x.dtype != dtype or not x.is_contiguous():
                raise ValueError(f"Chain.load(): a contiguous {dtype} tensor of shape {shape} is needed, not {x.dtype} {tuple(x.shape)}")
            return x
        self._vars = dev(variables, (wp.n_vars, n, 4) if by_variable else (n, wp.n_vars, 4), torch.int32)
        self._flow, self._swap = dev(flow, (n, F, 32), torch.int32), dev(swap, (n, F), torch.uint8)
        self.acc = torch.ones(n, dtype=torch.uint8, device=self.device)
        if check:
            self.bad_row, self.bad_flow = self._new(n), self._new(n)
            self.ctx.circuit_check(wp, self._vars, n, self.acc, self.bad_row)
            self.ctx.circuit_flow(wp, self._vars, n, self._flow, self._swap, self.acc, self.bad_flow)
        self._gather_inputs()
        self.done = {"witness"}

    def evaluate(self, inputs, flow_in=None, check=True, by_variable=False, mask=None):
        """The witnesses computed on the device in the place of load(), for a Circuit made with hints
        (Context.circuit_eval): inputs uint32[n, n_inputs, 4], the free inputs of every witness; flow_in uint32[n, n_flow,
        32] or None: the input halves with neither a wire nor a link (the other words are not read); mask uint8[n] or None:
        0 skips a witness.  numpy arrays, or device tensors.  The variables ([n_vars, n, 4] with by_variable: the context's
        witness_layout option is "by_variable"), the flow and the swap bytes are the chain's own, prefilled with `fill`
        where flow_in gives no word: a skipped witness keeps the prefill.  acc is cleared, and bad_input [n] names the
        smallest slot, where an input word is not below P (all ones: none).  check=True: then Context.circuit_check and
        circuit_flow as in load(): acc, bad_row, bad_flow.  Not with aggregate."""
        import torch
        if self.aggregate:
            raise ValueError("Chain.evaluate() is not for aggregate=True")
        n, wp = self.n, self.program
        n_inputs = wp.eval_info()[0]
        F = wp.shape.flow_count

        def dev(x, shape, dtype):
            if not torch.is_tensor(x):
                x = np.ascontiguousarray(x, np.uint8 if dtype == torch.uint8 else np.uint32)
                x = torch.from_numpy(x if dtype == torch.uint8 else x.view(np.int32)).to(self.device)
            if tuple(x.shape) != shape or x.dtype != dtype or not x.is_contiguous():
                raise ValueError(f"Chain.evaluate(): a contiguous {dtype} tensor of shape {shape} is needed, not {x.dtype} {tuple(x.shape)}")
            return x
        d_inputs = dev(inputs, (n, n_inputs, 4), torch.int32) if n_inputs else None
        self._vars = self._new(*((wp.n_vars, n, 4) if by_variable else (n, wp.n_vars, 4)))
        self._flow, self._swap = self._new(n, F, 32), self._new(n, F, flag=True)
        if flow_in is not None:
            free = torch.from_numpy(np.repeat(wp.flow_free, 8, axis=1)).to(self.device)     # [F, 16]: the words that are read
            self._flow[:, :, :16] = torch.where(free[None], dev(flow_in, (n, F, 32), torch.int32)[:, :, :16], self._flow[:, :, :16])
        self.acc = torch.ones(n, dtype=torch.uint8, device=self.device) if mask is None else dev(mask, (n,), torch.uint8).clone()
        self.bad_input = self._new(n)
        self.ctx.circuit_eval(wp, d_inputs, n, self._vars, self._flow, self._swap, self.acc, self.bad_input)
        if check:
            self.bad_row, self.bad_flow = self._new(n), self._new(n)
            self.ctx.circuit_check(wp, self._vars, n, self.acc, self.bad_row)
            self.ctx.circuit_flow(wp, self._vars, n, self._flow, self._swap, self.acc, self.bad_flow)
        self._gather_inputs()
        self.done = {"witness"}

    def _gather_inputs(self):
        """The statements, while the variables are there (trace() drops them): Context.circuit_inputs into the chain's own
        tensor [n, num_input, 5]."""
        import torch
        self._packed = None
        self._inputs = torch.zeros((self.n, self.program.num_input, 5), dtype=torch.int32, device=self.device)
        self.ctx.circuit_inputs(self.program, self._vars, self.n, self._inputs)

    def inputs(self):
        """-> the device tensor of the chain's own statements, int32[n, num_input, 5]: per witness the records (k,
        variables[k]) for k = 1 .. num_input, in the layout Context.verify_batch takes as d_inputs.  Written by witness(),
        load() or evaluate() on the context's stream (Context.circuit_inputs); a built program's are the three constants,
        followed by the own inputs of the proofs it verifies where it was built with n_fixed (with aggregate: per group,
        copy after copy)."""
        if self._inputs is None:
            raise ValueError("Chain.inputs() needs witness(), load() or evaluate() first")
        return self._inputs

    def verify(self, cfg):
        """pack(), if not yet packed, then ONE verifying call on the packed pair with the chain's own statements
        (Context.verify_batch with d_inputs = inputs()): neither the proofs nor the statements leave the device.
        -> (d_accept, d_reason) uint8[n], complete after synchronize() / release_to_torch(); a slot that pack() left empty (ok
        = 0) is rejected with the parser's reason."""
        d_inputs = self.inputs()
        if self._packed is None:
            self._packed = self.pack()
        d_blob, d_offsets = self._packed
        d_accept, d_reason = self._new(self.n, flag=True), self._new(self.n, flag=True)
        self.ctx.verify_batch(d_blob, d_offsets, self.n, d_accept, d_reason, cfg=cfg, d_inputs=d_inputs, n_inputs=int(d_inputs.shape[1]))
        return d_accept, d_reason

    def trace(self, plonk=True, poseidon=True, ops=True):
        """Context.witness_trace (an output may be skipped), then the blob, the variables and the flow are dropped: torch's
        stream is first made to wait for the context, so that a reuse of their memory is ordered behind the kernels reading it."""
        self._need("trace", "witness")
        n = self.n
        self.plonk = self._new(n, 12, 1 << self.lp) if plonk else None
        self.poseidon = self._new(n, 48, 1 << self.lq) if poseidon else None
        self.ops = self._new(n, max(self.n_ops, 1)) if ops else None
        trace = self.ctx.witness_trace_groups if self.aggregate else self.ctx.witness_trace
        trace(self.program, self._vars, self.acc, n, d_plonk=self.plonk, d_poseidon=self.poseidon, d_ops=self.ops, d_flow=self._flow,
              d_flow_swap=self._swap)
        self.ctx.release_to_torch()
        self._blob = self._vars = self._flow = self._swap = None
        self.done = {"trace"}

    def _lead(self):
        return (self.program, self.plonk, self.poseidon, self.ops, self.int_plonk, self.int_poseidon, self.acc, self.n)

    def commit(self):
        """Context.witness_commit: trees 0-2, the draws, the interaction columns and sums, the channel, ok (and the caps)."""
        self._need("commit", "trace")
        n, b, lp, lq = self.n, self.log_blowup, self.lp, self.lq
        if self.roots is None:
            self.roots, self.draws, self.sums, self.channel = self._new(n, 3, 8), self._new(n, 12), self._new(n, 2, 4), self._new(n, 16)
            self.int_plonk, self.int_poseidon = self._new(n, 8, 1 << lp), self._new(n, 8, 1 << lq)
            self.ok = self._new(n, flag=True)
            self.caps = self._new(n, 3, 2 << b, 8) if self.with_caps else None
        self.ctx.witness_commit(self.program, self.plonk, self.poseidon, self.ops, self.acc, n, b, self.roots, self.draws, self.int_plonk,
                                self.int_poseidon, self.sums, d_channel=self.channel, d_ok=self.ok, d_caps=self.caps)
        self.done.add("commit")

    def decommit(self, d_queries, d_values, d_n_values, d_witness, d_n_witness, caps=True):
        """Context.witness_decommit at d_queries uint32[n, n_queries] into the caller's buffers (capacities:
        witness_decommit_sizes); caps=False opens without the caps even where the chain keeps them."""
        self._need("decommit", "commit")
        self.ctx.witness_decommit(*self._lead(), self.log_blowup, d_queries, d_queries.shape[1], d_values, d_n_values, d_witness, d_n_witness,
                                  d_ok=self.ok, d_caps=self.caps if caps else None)

    def tree3(self):
        """Context.witness_tree3: the composition polynomial, its root (and cap), the OODS point, its samples; the channel moves on."""
        self._need("tree3", "commit")
        n = self.n
        if self.comp is None:
            L3 = composition_log_size(self.lp, self.lq)
            self.comp, self.root3, self.oods, self.samples3 = self._new(n, 8, 1 << L3), self._new(n, 8), self._new(n, 8), self._new(n, 8, 4)
            self.cap3 = self._new(n, 2 << self.log_blowup, 8) if self.with_caps else None
        self.ctx.witness_tree3(*self._lead(), self.log_blowup, self.sums, self.draws, self.channel, self.comp, self.root3, self.oods,
                               self.samples3, d_ok=self.ok, d_cap3=self.cap3)
        self.done.add("tree3")

    def sample(self, d_oods=None):
        """Context.witness_sample at d_oods uint32[n, 8], or at the point tree3() drew."""
        self._need("sample", "commit", *(() if d_oods is not None else ("tree3",)))
        if self.samples is None:
            self.samples = self._new(self.n, 134, 4)
        self.ctx.witness_sample(*self._lead(), self.oods if d_oods is None else d_oods, self.samples, d_ok=self.ok)
        self.done.add("sample")

    def fri(self):
        """Context.witness_fri (log_last as given to the constructor): `after`, the quotient columns, the layers' roots and
        alphas, the inner layers, the last polynomial, low_degree (and fri_caps, with fri_sub_log); the channel moves on."""
        self._need("fri", "tree3", "sample")
        if self.log_last is None:
            raise ValueError("Chain.fri() needs log_last")
        n, b, last = self.n, self.log_blowup, self.log_last
        if self.quot is None:
            sz = fri_sizes(self.lp, self.lq, b, last)
            ni = sz["n_inner"]
            self.after, self.quot, self.fri_roots, self.alphas = self._new(n, 4), self._new(n, sz["quot_words"]), self._new(n, 1 + ni, 8), self._new(n, 1 + ni, 4)
            self.layers, self.last_poly = self._new(n, max(sz["layer_words"], 1)), self._new(n, 1 << last, 4)
            self.low_degree = self._new(n, flag=True)
            if self.fri_sub_log:
                self.fri_caps = self._new(max(fri_cap_sizes(sz["sizes"], b, last, self.fri_sub_log, n)[0], 1))
        self.ctx.witness_fri(*self._lead(), b, last, self.comp, self.oods, self.samples, self.samples3, self.channel, self.after, self.quot,
                             self.fri_roots, self.alphas, self.layers, self.last_poly, self.low_degree, d_ok=self.ok,
                             sub_log=self.fri_sub_log, d_caps=self.fri_caps, tail_log=self.fri_tail_log)
        self.done.add("fri")

    def pow(self, pow_bits, n_queries, start=0, max_tries=0):
        """Context.pow_grind, then Context.draw_queries: the nonce [n, 2], the queries [n, n_queries] at the largest column's
        log size (fri_sizes' sizes[0]) and queries_low, the same at max(lp, lq) + log_blowup, where trees 0-2 are opened; the
        channel moves on, ok is cleared where the search is exhausted.  pow_bits is remembered for the proof's header."""
        self._need("pow", "fri")
        n = self.n
        self.pow_bits = pow_bits
        if self.nonce is None or self.queries.shape[1] != n_queries:
            self.nonce, self.queries, self.queries_low = self._new(n, 2), self._new(n, n_queries), self._new(n, n_queries)
        M = fri_sizes(self.lp, self.lq, self.log_blowup, self.log_last)["sizes"][0]
        self.ctx.pow_grind(pow_bits, n, self.ok, self.channel, self.nonce, start=start, max_tries=max_tries)
        self.ctx.draw_queries(n, n_queries, M, max(self.lp, self.lq) + self.log_blowup, self.channel, self.queries, self.queries_low, d_mask=self.ok)
        self.done.discard("open")
        self.done.discard("fri_open")
        self._packed = None
        self.done.add("pow")

    def open(self, caps=True):
        """The openings of trees 0-3 at the queries pow() drew: Context.witness_decommit at queries_low into values [n, v0 +
        v1 + v2], n_values [n, 3], witness_nodes [n, 3, w, 8], n_witness [n, 3] (witness_decommit_sizes), and
        Context.decommit_tree of tree 3 (the composition's eight columns) at queries into values3, n_values3 [n], witness3,
        n_witness3 [n] (decommit_sizes); caps=False opens without the caps even where the chain keeps them."""
        self._need("open", "pow")
        n, b, nq = self.n, self.log_blowup, self.queries.shape[1]
        L3 = composition_log_size(self.lp, self.lq)
        if self.values is None or "open" not in self.done:
            vcaps, wcap = witness_decommit_sizes(self.program, b, nq)
            v3, w3 = decommit_sizes([(L3, 8)], b, nq)
            self.values, self.n_values = self._new(n, sum(vcaps)), self._new(n, 3)
            self.witness_nodes, self.n_witness = self._new(n, 3, wcap, 8), self._new(n, 3)
            self.values3, self.n_values3, self.witness3, self.n_witness3 = self._new(n, v3), self._new(n), self._new(n, w3, 8), self._new(n)
        self.decommit(self.queries_low, self.values, self.n_values, self.witness_nodes, self.n_witness, caps=caps)
        cap3 = self.cap3 if caps else None
        self.ctx.decommit_tree([{"log_size": L3, "d_cols": self.comp, "n_cols": 8}], n, b, self.queries, nq, self.values3, self.n_values3,
                               self.witness3, self.n_witness3, d_mask=self.ok, cap_mode=CAP_NONE if cap3 is None else CAP_READ, d_cap=cap3)
        self.done.add("open")

    def fri_open(self, caps=True):
        """The openings of the FRI layer trees at the queries pow() drew: Context.fri_open on quot and layers into fri_witness
        [n, T, v, 4], n_fri_witness [n, T], fri_hash_witness [n, T, w, 8], n_fri_hash_witness [n, T] (T = 1 + n_inner;
        fri_open_sizes).  From fri_caps where the chain keeps them (fri_sub_log); otherwise, and with caps=False, every tree
        is hashed again."""
        self._need("fri_open", "pow")
        n, b, last, nq = self.n, self.log_blowup, self.log_last, self.queries.shape[1]
        sz = fri_sizes(self.lp, self.lq, b, last)
        T = 1 + sz["n_inner"]
        if self.fri_witness is None or "fri_open" not in self.done:
            vcap, wcap = fri_open_sizes(sz["sizes"], b, last, nq)
            self.fri_witness, self.n_fri_witness = self._new(n, T, vcap, 4), self._new(n, T)
            self.fri_hash_witness, self.n_fri_hash_witness = self._new(n, T, wcap, 8), self._new(n, T)
        d_caps = self.fri_caps if caps else None
        self.ctx.fri_open(self.quot, self.layers, sz["sizes"], b, last, n, self.queries, nq, self.fri_witness, self.n_fri_witness,
                          self.fri_hash_witness, self.n_fri_hash_witness, d_mask=self.ok, sub_log=self.fri_sub_log if d_caps is not None else 0,
                          d_caps=d_caps)
        self.done.add("fri_open")

    def proofs(self):
        """-> per proof the serialised PlonkWithPoseidonProof (proof_bytes), None where ok is 0.  Assembled on the host from
        numpy(): synchronises."""
        self._need("proofs", "open", "fri_open")
        a = self.numpy()
        b, last, nq = self.log_blowup, self.log_last, self.queries.shape[1]
        vat = np.cumsum([0] + witness_decommit_sizes(self.program, b, nq)[0])
        out = []
        for k in range(self.n):
            if not a["ok"][k]:
                out.append(None)
                continue
            openings = [(a["values"][k, vat[t]:vat[t] + a["n_values"][k, t]], a["witness_nodes"][k, t, :a["n_witness"][k, t]]) for t in range(3)]
            openings.append((a["values3"][k, :a["n_values3"][k]], a["witness3"][k, :a["n_witness3"][k]]))
            layers = [(a["fri_witness"][k, t, :a["n_fri_witness"][k, t]], a["fri_hash_witness"][k, t, :a["n_fri_hash_witness"][k, t]],
                       a["fri_roots"][k, t]) for t in range(a["fri_roots"].shape[1])]
            out.append(proof_bytes(self.lp, self.lq, a["sums"][k], (self.pow_bits, b, last, nq), np.concatenate([a["roots"][k], a["root3"][k][None]]),
                                   np.concatenate([a["samples"][k], a["samples3"][k]]), openings, a["nonce"][k], layers, a["last_poly"][k], last))
        return out

    def pack(self, exact=False):
        """-> (d_blob uint8, d_offsets int64[n + 1]) on the device: the serialised proofs in the verifier's blob layout
        (Context.proof_pack pointed into the chain's own tensors), proof k at d_blob[d_offsets[k]:d_offsets[k + 1]], an empty
        slot where ok is 0.  exact=False: the blob is sized by the capacities (proof_bytes_bound) and nothing synchronises;
        exact=True: an offsets-only call, d_offsets[n] is read (synchronises), the blob holds exactly the proofs.  torch's
        stream is made to wait for the context, so the pair may be read with torch as well as handed to a Context call."""
        import torch
        self._need("pack", "open", "fri_open")
        n, b, last, nq = self.n, self.log_blowup, self.log_last, self.queries.shape[1]
        T = self.fri_roots.shape[1]
        vcaps = witness_decommit_sizes(self.program, b, nq)[0]
        vat = np.cumsum([0] + vcaps)
        wcap, v3, w3 = self.witness_nodes.shape[2], self.values3.shape[1], self.witness3.shape[1]
        fv, fw = self.fri_witness.shape[2], self.fri_hash_witness.shape[2]
        parts = ProofParts(self.lp, self.lq, self.pow_bits, b, last, nq, T, *(t.data_ptr() for t in (
            self.sums, self.roots, self.root3, self.samples, self.samples3, self.nonce, self.fri_roots, self.last_poly)))
        for t in range(3):
            parts.values[t] = proof_list(self.values, int(vat[3]), self.n_values, 3, vcaps[t], items_at=int(vat[t]), count_at=t)
            parts.witness[t] = proof_list(self.witness_nodes, 3 * wcap * 8, self.n_witness, 3, wcap, items_at=t * wcap * 8, count_at=t)
        parts.values[3] = proof_list(self.values3, v3, self.n_values3, 1, v3)
        parts.witness[3] = proof_list(self.witness3, w3 * 8, self.n_witness3, 1, w3)
        parts.fri_witness = proof_list(self.fri_witness, T * fv * 4, self.n_fri_witness, T, fv)
        parts.fri_hash_witness = proof_list(self.fri_hash_witness, T * fw * 8, self.n_fri_hash_witness, T, fw)
        d_offsets = torch.full((n + 1,), -1 if self.fill else 0, dtype=torch.int64, device=self.device)
        if exact:
            self.ctx.proof_pack(parts, n, None, d_offsets, d_mask=self.ok)
            self.ctx.release_to_torch()
            size = int(d_offsets[n].item())
        else:
            size = n * proof_bytes_bound(last, T, vcaps + [v3] + [wcap] * 3 + [w3] + [fv, fw] * T)
        d_blob = torch.full((max(size, 4),), self.fill & 0xFF, dtype=torch.uint8, device=self.device)[:size]
        self.ctx.proof_pack(parts, n, d_blob, d_offsets, d_mask=self.ok)
        self.ctx.release_to_torch()
        return d_blob, d_offsets

    def numpy(self):
        """Synchronises -> {name: array} of every tensor allocated so far: uint32 views, the flags uint8; ops cut to the
        program's n_witness_ops."""
        self.ctx.synchronize()
        out = {}
        for name in _WRITTEN:
            t = getattr(self, name)
            if t is not None:
                out[name] = t.cpu().numpy() if name in _FLAGS else t.cpu().numpy().view(np.uint32)
        if "ops" in out:
            out["ops"] = out["ops"][:, :self.n_ops]
        return out
