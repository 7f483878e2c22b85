// astar_trace_parent.hpp -- the canonical parent of one cell of a finished grid-A* field, shared by the walk of astar_tile.hip
// (tsa_backtrace_wave computes it for every cell of a tile at once) and by the host test that checks the rule
// (tests/cpp/astar_trace_parent_test.cpp): both compile this text.
#pragma once

namespace rna {

#ifdef __HIPCC__
#define RNA_TRACE_HD __host__ __device__ __forceinline__
#else
#define RNA_TRACE_HD inline   // a host compiler alone
#endif

constexpr unsigned TSA_PARENT_NONE = 8u;   // code of a cell the walk cannot leave: unreached, or no neighbour qualifies
constexpr unsigned TSA_PARENT_COST_S = 1000u, TSA_PARENT_COST_D = 1414u;   // (= COST_S, COST_D of astar_tile.hip, asserted there)

// Neighbour k of a cell, k = 0..7 in the order of the linear index j * rows + i: (i-1, j-1) (i, j-1) (i+1, j-1) (i-1, j) (i+1, j)
// (i-1, j+1) (i, j+1) (i+1, j+1) -- the numbering of the neighbour-mask bits.  Field words are u = KU - g, 0 = unreached, so the
// parent of c over move k has u(n) == u(c) + w_k.  The code of a cell: the lowest k whose move bit is set in the cell's own mask
// byte mc, with u(n) != 0 and u(n) == u(c) + w_k; TSA_PARENT_NONE if there is none or the cell itself is unreached.
// (All eight tests are evaluated and joined as bits: no branches, and on the GPU no dependent chain from one k to the next.)
RNA_TRACE_HD unsigned tsa_parent_code(unsigned uc, unsigned mc, unsigned n0, unsigned n1, unsigned n2, unsigned n3, unsigned n4, unsigned n5,
                                      unsigned n6, unsigned n7) {
  const unsigned s = uc + TSA_PARENT_COST_S, d = uc + TSA_PARENT_COST_D;
  unsigned h = 0u;
  h |= ((n0 != 0u) & (n0 == d)) ? 1u : 0u;
  h |= ((n1 != 0u) & (n1 == s)) ? 2u : 0u;
  h |= ((n2 != 0u) & (n2 == d)) ? 4u : 0u;
  h |= ((n3 != 0u) & (n3 == s)) ? 8u : 0u;
  h |= ((n4 != 0u) & (n4 == s)) ? 16u : 0u;
  h |= ((n5 != 0u) & (n5 == d)) ? 32u : 0u;
  h |= ((n6 != 0u) & (n6 == s)) ? 64u : 0u;
  h |= ((n7 != 0u) & (n7 == d)) ? 128u : 0u;
  h &= mc & 0xffu;
  if (uc == 0u) h = 0u;
  return (unsigned)__builtin_ctz(h | (1u << TSA_PARENT_NONE));
}

}  // namespace rna
