"""Instruction-cost ceiling of the Poseidon2 permutation on one MI355X (bench.py: valu.ceiling_perms_per_s).

Dynamic VALU instruction mix of ONE wave-level call of rsv::poseidon2() (64 permutations), derived from the source
(recursive-stwo_amd/csrc/poseidon2.hpp) and checked against the hardware count:

  S-box with its pre-reduction, x -> x^5 (142 of them: 8 full rounds x 16 + 14 partial rounds x 1), in centred form,
  entered through centre_rc (the sign-mask select, no v_min)
      fold2 + round constant (moved by 2^30) + centred representative in one: lshr, v_add3_u32 (hi + lo/2 - c, the literal
      in an SGPR), v_ashrrev_i32 (the sign of a = t - c), v_xad_u32 ((sign ^ 0xC0000000) + a, the mask an inline constant)
      + pow5c, every product v_mad_i64_i32 with a signed SGPR-pair addend (KP = -P * 2^32, KN = -P * 2^31, KQ = P * 2^31):
             [add (2x)] + [mad(2x, x, KP), lshr, add] + [mad(s1, s1, KN), alignbit, and, add] + [mad(2x, c4, KQ), lshr, add]
      = 9 fast, 1 v_add3_u32, 1 v_xad_u32, 2 v_mad_i64_i32 a * b + SGPR pair, 1 v_mad_i64_i32 a * a + SGPR pair,
        1 v_alignbit_b32
      (before the sign-mask entry: fold2's add, two literal adds and a v_min, pow5c's centring subtract: 12 fast
      and 1 v_min_u32, 3.0 cycles more than now; before the centred form: [add, mad (SGPR pair), lshr, add] +
      [v_mad_i64_i32, alignbit, and, add, add-literal, min] + [mad, lshr, add]: 12 fast, 2 min, 42.0 cycles; before the
      signed square: 14 fast, 3 min, 3 mads without addend per S-box, 47.2 cycles)
  full-round linear layer, column sums first (9 of them; none carries round constants: they are literals of the S-box
  reduction): group g of circ(2M4, M4, M4, M4) s is M4 (s_g + X), X the column sums
      doubled column sums X2_j: 1 mad (no addend) + 3 mad (addend), four columns                                = 16
      z = 2 s + X2: 16 mad (addend)                                                                             = 16
      M4 on 64-bit inputs: 8 lshl_add_u64 per group                                                             = 32
      (before: M4 per group on 32-bit inputs, 2 mad (no addend) + 4 mad (addend) + 4 lshl_add_u64, and the sums of its
      outputs afterwards, 12 + 16 lshl_add_u64: 8 + 16 + 44 = 68 per layer)
  partial rounds (14 = single 0, pairs (1,2) .. (11,12), single 13; a pair forms round R + 1's words straight from
  round R's inputs, so 15 words are folded once per pair instead of twice)
      single: 2 mad (no addend) + 14 + 1 + 15 mad (addend) + 1 lshl_add_u64, 16 fold2 = 32 fast
      pair:   4 mad (no addend) + 28 + 2 + 1 + 30 mad (addend) + 2 lshl_add_u64, 18 fold2 = 36 fast
              (against two singles: -28 fast, +1 mad with addend — the round's sum S folded once and added as 30 S)
  output: 16 x (lshr, add, add-literal, min)
  the half-output instances poseidon2_half_t<HI, PACE> (every hash of the verify path): the last layer forms all four
  column sums but z and M4 for the two kept groups only, 4 mad (no addend) + 20 mad (addend) + 16 lshl_add_u64 = 40 (before:
  four M4 and the sums, 8 + 16 + 36 = 60), and eight outputs: HALF_DELTA below

  class                      count   cycles/instr at 4 waves/SIMD, expressed at 2.4 GHz (tools/valu_lab.hip, measured r2;
                                     the rows of the signed S-boxes measured with it, 8 waves/SIMD in brackets)
  fast  (add/sub/lshr/ashr/and) 1578 2.50     (a 32-bit literal operand does not change the class: 2.52; v_ashrrev_i32 2.44-2.47,
                                              profiles/r3_valu_lab_*)
  v_min_u32                     16   4.27     (the output canonicalisations)
  v_add3_u32                   142   4.42     (4.54 / 4.29 at 4 / 6 waves per SIMD, profiles/r3_valu_lab_*; 4.22 at 8, r14)
  v_xad_u32                    142   4.38     (4.44 / 4.32 at 4 / 6 waves per SIMD; 4.20 at 8)
  v_mad_u64_u32, no addend      64   4.54
  v_lshl_add_u64               302   4.48
  v_mad_u64_u32, with addend   678   5.10     (SGPR multiplier or live 64-bit addend: 5.05-5.15)
  v_mad_i64_i32, SGPR pair     284   4.51     (4.37; v_mad_u64_u32 with an SGPR-pair addend in the same run: 4.51 (4.37))
  v_mad_i64_i32 square, pair   142   4.30     (4.27; one VGPR operand read twice: the square without addend 4.33 (4.26))
  v_alignbit_b32               142   4.40     (4.20)
  total                       3490            = the static count: the function is straight-line code since the constants
                                              became literals; the 142 v_add3_u32 take their constant from an SGPR, so the
                                              function also holds 142 + 32 s_mov_b32 (SALU, not in the mix)
                                              (before: 4 428 with 736 addend-mads, 15 650 cycles, 10.05 G/s;
                                              before the paired partial rounds: 4 398, 2 456 fast and 564 addend-mads,
                                              15 129 cycles, 10.40 G/s; before the signed square: 4 236, 2 288 fast, 442
                                              v_min, 526 mads without addend, 14 739 cycles, 10.67 G/s; before the centred
                                              S-box: 3 952, 300 v_min, 242 mads without addend, 142 v_mad_i64_i32 without
                                              addend, 142 v_mad_u64_u32 with an SGPR-pair addend, 14 011 cycles, 11.23 G/s;
                                              before the sign-mask entry: 3 810, 2 004 fast, 158 v_min, no v_add3_u32 or
                                              v_xad_u32, 13 399 cycles, 11.74 G/s; before the column sums went
                                              first: 3 526, 100 mads without addend, 570 with, 410 v_lshl_add_u64,
                                              12 977 cycles, 12.12 G/s)

=> 12 880 cycles-at-2.4-GHz per 64 permutations per SIMD => 1024 SIMDs x 2.4e9 / 12 880 x 64 = 12.21 G permutations/s;
a half-output call 12 674 cycles (before: 12 847, -1.35 %).
(The lab's "cycles at 2.4 GHz" are wall time x 2.4 GHz.  Round 5 separated clock from issue cost (tools/valu_clock.sh,
profiles/r5_valu_lab_*): under the lab's dense VALU load GRBM_GUI_ACTIVE holds 2.35-2.40 GHz — v_and_b32 at 4 waves per
SIMD: 2.242 ms at 2.383 GHz for 2 097 152 wave-instructions per SIMD = 2.55 REAL cycles each — so the fast class's 2.5
against the nominal 2 (MI355X_MICROARCH.md) is issue overhead of the SIMD, not a power state; one wave alone issues every
5.1 cycles.  The per-wave clock64 column of the lab shows the arbiter instead: it favours a SIMD's oldest wave, the waves
finish one after the other, and only the longest-lived one spans the launch.)

Usage: python tools/perm_ceiling.py [path/to/asm]   — with an assembly listing (hipcc -S --cuda-device-only) it also
prints the STATIC opcode histogram of rsv::poseidon2 and of the four poseidon2_half_t instances as a cross-check of the class
membership."""
import collections
import re
import sys

MIX = [("fast", 1578, 2.50), ("v_min_u32", 16, 4.27), ("v_add3_u32", 142, 4.42), ("v_xad_u32", 142, 4.38), ("v_mad_u64_u32 (no addend)", 64, 4.54),
       ("v_lshl_add_u64", 302, 4.48), ("v_mad_u64_u32 (addend)", 678, 5.10), ("v_mad_i64_i32 (SGPR-pair addend)", 284, 4.51),
       ("v_mad_i64_i32 square (SGPR-pair addend)", 142, 4.30), ("v_alignbit_b32", 142, 4.40)]
# a half-output call against the mix above: the tail in place of the last layer (28 -> 20 mads with addend, 32 -> 16
# v_lshl_add_u64) and eight outputs instead of sixteen (3 fast and 1 v_min each)
HALF_DELTA = {"fast": -24, "v_min_u32": -8, "v_mad_u64_u32 (addend)": -8, "v_lshl_add_u64": -16}
# the same two rows of the form before the column sums went first (sums after M4), for the modelled saving
MIX_BEFORE = {"v_mad_u64_u32 (no addend)": 100, "v_lshl_add_u64": 410, "v_mad_u64_u32 (addend)": 570}
HALF_DELTA_BEFORE = {"fast": -24, "v_min_u32": -8, "v_lshl_add_u64": -8}
SIMDS, LAB_GHZ = 1024, 2.4


def ceiling():
    cycles = sum(n * c for _, n, c in MIX)
    return SIMDS * LAB_GHZ * 1e9 / cycles * 64.0, cycles, sum(n for _, n, _ in MIX)


def priced(base=None, delta=None):
    """(instructions, cycles) of MIX with the counts of `base` replaced and those of `delta` added"""
    rows = [(name, (base or {}).get(name, n) + (delta or {}).get(name, 0), c) for name, n, c in MIX]
    return sum(n for _, n, _ in rows), sum(n * c for _, n, c in rows)


def histogram(listing, symbol):
    m = re.search(r"\n" + symbol + r":.*?s_setpc_b64", listing, re.S)
    return collections.Counter(l.split()[0] for l in m.group(0).splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";")))


def main():
    perms, cycles, insts = ceiling()
    print(f"{insts} VALU instructions, {cycles:.0f} cycles@2.4GHz per wave-level call -> ceiling {perms / 1e9:.2f} G permutations/s")
    (h_insts, h_cycles), (b_insts, b_cycles) = priced(delta=HALF_DELTA), priced(MIX_BEFORE, HALF_DELTA_BEFORE)
    print(f"half-output call: {h_insts} VALU instructions, {h_cycles:.0f} cycles; with the sums after M4 {b_insts} and {b_cycles:.0f}: "
          f"{h_insts - b_insts} instructions, {100 * (h_cycles / b_cycles - 1):.2f} % cycles")
    if len(sys.argv) > 1:
        s = open(sys.argv[1]).read()
        ops = histogram(s, "_ZN3rsv9poseidon2ENS_7State16E")
        print("static histogram of rsv::poseidon2 (straight-line code: equals the dynamic count):", ops.most_common(12))
        print(f"static VALU instructions: {sum(n for op, n in ops.items() if op.startswith('v_'))} (the mix: {insts})")
        for hi in (0, 1):
            for pace in (1, 0):
                ops = histogram(s, f"_ZN3rsv16poseidon2_half_tILb{hi}ELb{pace}EEENS_5Hash8ENS_7State16E")
                print(f"poseidon2_half_t<{hi}, {pace}>: v_mad_u64_u32 {ops['v_mad_u64_u32']}, v_lshl_add_u64 {ops['v_lshl_add_u64']}, "
                      f"v_min_u32 {ops['v_min_u32_e32'] + ops['v_min_u32']}, "
                      f"static VALU instructions {sum(n for op, n in ops.items() if op.startswith('v_'))} (the mix: {h_insts})")


if __name__ == "__main__":
    main()
