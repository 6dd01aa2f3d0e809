// wfa_pk16.hpp -- two 16-bit offsets per register: the packed WF_NEXT shared by wfa_wide_kernel (the wide rows' interior) and
// the packed instance of wfa_duo_kernel (rings held as pairs of diagonals).  v_pk_max_u16 / v_pk_add_u16 / v_pk_sub_u16 with
// clamp / v_pk_min_u16 issue at the rate of one 32-bit vector instruction (profiles/r02_valu_issue_probe.txt): two diagonals per
// instruction.  Offsets must stay below 4 096 -- reads under 2 048 bases -- so that blk_word() fits a halfword.
#pragma once
#include "wfa_device.hpp"

namespace wfa {

typedef unsigned short wide_us2 __attribute__((ext_vector_type(2)));
WFA_DEV wide_us2 wide_pk(uint32_t x) { return __builtin_bit_cast(wide_us2, x); }
WFA_DEV uint32_t wide_u32(wide_us2 x) { return __builtin_bit_cast(uint32_t, x); }
WFA_DEV wide_us2 wide_max(wide_us2 a, wide_us2 b) { return __builtin_elementwise_max(a, b); }
// (`one` = (1, 1) from a register the compiler cannot see through: it turns min(a, 1) into two compares, two selects and a permute otherwise)
WFA_DEV wide_us2 wide_ind(wide_us2 a, wide_us2 one) { return __builtin_elementwise_min(a, one); }                             // 1 where a != 0
WFA_DEV wide_us2 wide_lt(wide_us2 a, wide_us2 b, wide_us2 one) { return wide_ind(__builtin_elementwise_sub_sat(b, a), one); }  // 1 where a < b
// WF_NEXT of two neighbouring diagonals whose sources need no rejection (wfa.go:572-699; the decisions as blk_word_asm() takes them: the mismatch
// wins iff x1 >= max(Isk, Dsk), else the insertion iff Isk >= Dsk; backTrace's recomputed pre-extension offset is the M offset itself).
// DUO = false (wfa_wide_kernel): an absent cell's word is 0.  DUO = true (wfa_duo_kernel): the word of an absent cell is what
// blk_word_asm() gives it, 3 -- every source 0, both ">=" decisions set -- so that the packed rings write the arena byte for byte as
// the 32-bit ones do; and the four decisions go in under the offset with one v_pk_mad_u16 each (w = 2 w + bit), where hipcc makes a
// shift and an add of every one.
template <bool DUO = false>
WFA_DEV void wide_next2(wide_us2 a, wide_us2 b, wide_us2 c, wide_us2 d, wide_us2 x, wide_us2 one, uint32_t &M2, uint32_t &I2, uint32_t &D2, uint32_t &W2) {
    const wide_us2 mi = wide_max(a, b), Isk = mi + wide_ind(mi, one), Dsk = wide_max(c, d), x1 = x + wide_ind(x, one);
    const wide_us2 t = wide_max(Isk, Dsk), Msk = wide_max(t, x1);
    const wide_us2 iext = wide_lt(a, b, one), dext = wide_lt(c, d, one), fx = one - wide_lt(x1, t, one), fi = one - wide_lt(Isk, Dsk, one);
    if constexpr (DUO) {
        const auto mad2 = [](uint32_t w, wide_us2 bit) {  // 2 w + bit in both halves (the constant's low half for both: op_sel_hi 0)
            uint32_t r;
            asm("v_pk_mad_u16 %0, %1, 2, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(w), "v"(wide_u32(bit)));
            return r;
        };
        W2 = mad2(mad2(mad2(mad2(wide_u32(Msk), iext), dext), fx), fi);
    } else {
        wide_us2 w = Msk + Msk + iext;
        w = w + w + dext, w = w + w + fx, w = w + w + fi;
        w &= (wide_us2)(0) - wide_ind(Msk, one);  // (no cell: no word)
        W2 = wide_u32(w);
    }
    M2 = wide_u32(Msk), I2 = wide_u32(Isk), D2 = wide_u32(Dsk);
}

}  // namespace wfa
