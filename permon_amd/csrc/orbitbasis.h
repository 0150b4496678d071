// Symmetry-adapted basis of a class whose touched dofs carry all 48 signed coordinate permutations of the cube (orbitbasis.hip, host only)
#pragma once
#include <string>
#include <vector>

#define OAB_NIRREP 10 // A1g A2g Eg T1g T2g A1u A2u Eu T1u T2u
#define OAB_NOP 48

// The basis functions are numbered orbit after orbit (orbits in the order of their first position), inside an orbit irrep after irrep, copy after copy,
// partner after partner: `row` below is that number (0 .. nc - 1), and orbit o owns the rows tbase[o] .. tbase[o] + osize[o] - 1 and as many positions.
struct oab_basis {
  int nc = 0, norb = 0;
  int d[OAB_NIRREP] = {0}, m[OAB_NIRREP] = {0};                 // dimension and multiplicity of every irrep: sum m d = nc
  std::vector<int>       osize, tbase;                          // per orbit
  std::vector<long long> toff;                                  // per orbit: its osize x osize table in tab (row-major: basis function x position)
  std::vector<int>       opos;                                  // [nc] the orbit's positions, ascending
  std::vector<int>       row_irrep, row_index, row_partner;     // [nc] per basis function: irrep, row of its copy in W^_irrep, partner a
  std::vector<double>    row_v, row_vs;                         // [3 nc] the copy's vector v_k (dimension d, zero-padded); the same times sqrt(|O| / d) (set-up of W^_i)
  std::vector<double>    tab;
};

// ops: (ax[3], fl[3]) per operation.  Returns true and fills `out` when the basis was built and passed its checks; false with the reason in `why` otherwise
// (fewer than 48 operations, an action that does not tell the operations apart, a failed check).
bool oab_build(int nsym, int nc, const int *posmap, const signed char *sign, const int *ops, oab_basis &out, std::string &why);
