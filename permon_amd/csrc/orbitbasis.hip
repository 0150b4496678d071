// Symmetry-adapted basis for the class-shared explicit operators in orbit storage (host code).
//
// W_c = K^+[U_c, U_c] commutes with the 48 signed coordinate permutations T(g) of the cube, (T(g) x)[g p] = s_g(p) x[p].  In a basis that transforms under
// the ten irreducible representations rho_i of that group (dimensions 1, 1, 2, 3, 3, each even and odd), with the SAME matrices rho_i in every orbit, Schur's
// lemma gives  U' W U = (+)_i (W^_i (x) I_{d_i}):  one application costs sum_i 2 m_i^2 d_i flops per right-hand side on sum_i m_i^2 matrix entries.
//
// Irreps of g = (ax, fl), M[a][ax[a]] = fl[a]:  delta = det M, R = delta M, eps = sign of the permutation ax, E(M) = B^+ |M| B with
// B = [(1, 0); (-1/2, sqrt(3)/2); (-1/2, -sqrt(3)/2)].  Even: A1 = 1, A2 = eps, E = E(M), T1 = R, T2 = eps R; odd: the same times delta.
//
// Basis of the orbit of p: stabiliser H = {h : h p = p}, sigma(h) = s_h(p); Pi_i = (1 / |H|) sum_h sigma(h) rho_i(h) is an orthogonal projector whose rank is
// the multiplicity of irrep i in the orbit; v_k an orthonormal basis of its range;  phi_{k,a}(g p) = sqrt(d / |O|) s_g(p) (rho_i(g) v_k)_a.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "orbitbasis.h"
#include "pmh_internal.h"

namespace {
typedef long double real; // the tables are built in extended precision and rounded ONCE: every entry is correct to half a unit, the basis orthonormal to rounding
struct mat3 {
  real v[3][3];
};

mat3 mul(const mat3 &a, const mat3 &b, int d)
{
  mat3 c{};
  for (int i = 0; i < d; i++)
    for (int j = 0; j < d; j++) {
      real s = 0.0L;
      for (int k = 0; k < d; k++) s += a.v[i][k] * b.v[k][j];
      c.v[i][j] = s;
    }
  return c;
}

// the ten matrices of one operation
void irreps_of(const int *op, mat3 rho[OAB_NIRREP])
{
  const int *ax = op, *fl = op + 3;
  real       M[3][3] = {{0}};
  for (int a = 0; a < 3; a++) M[a][ax[a]] = fl[a];
  const real det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
  int          inv = 0;
  for (int a = 0; a < 3; a++)
    for (int b = a + 1; b < 3; b++) inv += ax[a] > ax[b];
  const real eps = (inv & 1) ? -1.0L : 1.0L;
  const real h = sqrtl(3.0L) / 2.0L, B[3][2] = {{1.0L, 0.0L}, {-0.5L, h}, {-0.5L, -h}};
  for (int i = 0; i < OAB_NIRREP; i++) memset(&rho[i], 0, sizeof(mat3));
  rho[0].v[0][0] = 1.0L, rho[1].v[0][0] = eps;
  for (int i = 0; i < 2; i++) // E = (2 / 3) B' |M| B
    for (int j = 0; j < 2; j++) {
      real s = 0.0L;
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) s += B[a][i] * fabsl(M[a][b]) * B[b][j];
      rho[2].v[i][j] = s * 2.0L / 3.0L;
    }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) rho[3].v[a][b] = det * M[a][b], rho[4].v[a][b] = eps * det * M[a][b];
  for (int i = 0; i < 5; i++)
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) rho[5 + i].v[a][b] = det * rho[i].v[a][b];
}
} // namespace

bool oab_build(int nsym, int nc, const int *posmap, const signed char *sign, const int *ops, oab_basis &out, std::string &why)
{
  static const int dims_of[OAB_NIRREP] = {1, 1, 2, 3, 3, 1, 1, 2, 3, 3};
  out = oab_basis();
  if (nsym != OAB_NOP || !ops) { // a subgroup restricts the irreps to reducible ones: the block structure fails
    why = "fewer than 48 operations";
    return false;
  }
  if (nc < 1) {
    why = "no touched dofs";
    return false;
  }
  std::vector<mat3> rho((size_t)OAB_NOP * OAB_NIRREP);
  for (int g = 0; g < OAB_NOP; g++) irreps_of(ops + 6 * g, &rho[(size_t)g * OAB_NIRREP]);
  // rho_i(g) rho_i(h) = rho_i(g h) against the group's own composition on the positions (h first, then g), identified on a sample of positions
  {
    const int        ns = std::min(nc, 256);
    std::vector<int> samp(ns);
    for (int t = 0; t < ns; t++) samp[t] = (int)((long long)nc * t / ns);
    std::map<std::vector<int>, int> id;
    std::vector<int>                key(2 * (size_t)ns);
    for (int g = 0; g < OAB_NOP; g++) {
      for (int t = 0; t < ns; t++) key[2 * t] = posmap[(size_t)g * nc + samp[t]], key[2 * t + 1] = sign[(size_t)g * nc + samp[t]];
      if (!id.emplace(key, g).second) {
        why = "the action on the touched dofs does not tell the operations apart";
        return false;
      }
    }
    for (int g = 0; g < OAB_NOP; g++)
      for (int h = 0; h < OAB_NOP; h++) {
        for (int t = 0; t < ns; t++) {
          const int q = posmap[(size_t)h * nc + samp[t]];
          key[2 * t] = posmap[(size_t)g * nc + q], key[2 * t + 1] = sign[(size_t)h * nc + samp[t]] * sign[(size_t)g * nc + q];
        }
        auto it = id.find(key);
        if (it == id.end()) {
          why = "the operations are not closed under composition";
          return false;
        }
        const int gh = it->second;
        for (int i = 0; i < OAB_NIRREP; i++) {
          const mat3 p = mul(rho[(size_t)g * OAB_NIRREP + i], rho[(size_t)h * OAB_NIRREP + i], dims_of[i]);
          for (int a = 0; a < dims_of[i]; a++)
            for (int b = 0; b < dims_of[i]; b++)
              if (!(fabsl(p.v[a][b] - rho[(size_t)gh * OAB_NIRREP + i].v[a][b]) <= 1e-15L)) {
                why = "the irreps' matrices do not follow the group's composition";
                return false;
              }
        }
      }
  }
  out.nc = nc;
  for (int i = 0; i < OAB_NIRREP; i++) out.d[i] = dims_of[i];
  out.opos.reserve(nc), out.row_irrep.reserve(nc), out.row_index.reserve(nc), out.row_partner.reserve(nc), out.row_v.reserve(3 * (size_t)nc);
  std::vector<char> seen((size_t)nc, 0);
  for (int p = 0; p < nc; p++) {
    if (seen[p]) continue;
    // the orbit's positions, ascending, each with the first operation that reaches it; the stabiliser
    std::vector<std::pair<int, int>> img;
    std::vector<int>                 H;
    for (int g = 0; g < OAB_NOP; g++) {
      const int q = posmap[(size_t)g * nc + p];
      if (q == p) H.push_back(g);
      if (!seen[q]) seen[q] = 1, img.emplace_back(q, g);
    }
    std::sort(img.begin(), img.end());
    const int no = (int)img.size();
    if (no * (int)H.size() != OAB_NOP) {
      why = "an orbit's size is not the index of its stabiliser";
      return false;
    }
    const int       tb = (int)out.opos.size();
    const long long to = (long long)out.tab.size();
    out.osize.push_back(no), out.tbase.push_back(tb), out.toff.push_back(to);
    for (auto &q : img) out.opos.push_back(q.first);
    out.tab.resize((size_t)to + (size_t)no * no, 0.0);
    int t = 0;
    for (int i = 0; i < OAB_NIRREP; i++) {
      const int d = dims_of[i];
      real      P[3][3] = {{0}};
      for (int h : H)
        for (int a = 0; a < d; a++)
          for (int b = 0; b < d; b++) P[a][b] += (real)sign[(size_t)h * nc + p] * rho[(size_t)h * OAB_NIRREP + i].v[a][b] / (real)H.size();
      real tr = 0.0L;
      for (int a = 0; a < d; a++) tr += P[a][a];
      const int rank = (int)lroundl(tr);
      if (rank < 0 || rank > d || fabsl(tr - rank) > 1e-12L) {
        why = "a stabiliser's average is no projector";
        return false;
      }
      // orthonormal basis of the range: Gram-Schmidt on the columns, the longest remaining one first
      real v[3][3] = {{0}};
      for (int k = 0; k < rank; k++) {
        int  best = -1;
        real bn = 0.0L, bc[3] = {0, 0, 0};
        for (int c = 0; c < d; c++) {
          real col[3] = {0, 0, 0};
          for (int a = 0; a < d; a++) col[a] = P[a][c];
          for (int j = 0; j < k; j++) {
            real dot = 0.0L;
            for (int a = 0; a < d; a++) dot += v[j][a] * col[a];
            for (int a = 0; a < d; a++) col[a] -= dot * v[j][a];
          }
          real nn = 0.0L;
          for (int a = 0; a < d; a++) nn += col[a] * col[a];
          if (nn > bn * (1.0L + 1e-9L)) bn = nn, best = c, memcpy(bc, col, sizeof(bc));
        }
        if (best < 0 || !(bn > 1e-12L)) {
          why = "a projector's range is smaller than its trace";
          return false;
        }
        for (int a = 0; a < d; a++) v[k][a] = bc[a] / sqrtl(bn);
      }
      for (int k = 0; k < rank; k++) {
        for (int a = 0; a < d; a++, t++) {
          if (t >= no) {
            why = "an orbit holds more basis functions than positions";
            return false;
          }
          out.row_irrep.push_back(i), out.row_index.push_back(out.m[i] + k), out.row_partner.push_back(a);
          for (int b = 0; b < 3; b++) out.row_v.push_back(b < d ? (double)v[k][b] : 0.0), out.row_vs.push_back(b < d ? (double)(v[k][b] * sqrtl((real)no / d)) : 0.0);
          for (int j = 0; j < no; j++) {
            const int    g = img[j].second;
            const mat3  &r = rho[(size_t)g * OAB_NIRREP + i];
            real         s = 0.0L;
            for (int b = 0; b < d; b++) s += r.v[a][b] * v[k][b];
            out.tab[(size_t)to + (size_t)t * no + j] = (double)(sqrtl((real)d / no) * (real)sign[(size_t)g * nc + p] * s);
          }
        }
      }
      out.m[i] += rank;
    }
    if (t != no) {
      why = "an orbit holds fewer basis functions than positions";
      return false;
    }
    // the orbit's table is orthonormal
    const double *T = out.tab.data() + to;
    for (int a = 0; a < no; a++)
      for (int b = a; b < no; b++) {
        double s = 0.0;
        for (int j = 0; j < no; j++) s += T[(size_t)a * no + j] * T[(size_t)b * no + j];
        if (!(std::fabs(s - (a == b ? 1.0 : 0.0)) <= 1e-14)) {
          why = "an orbit's table is not orthonormal";
          return false;
        }
      }
  }
  out.norb = (int)out.osize.size();
  long long tot = 0;
  for (int i = 0; i < OAB_NIRREP; i++) tot += (long long)out.m[i] * out.d[i];
  if (tot != nc || (int)out.opos.size() != nc) {
    why = "the multiplicities do not add up to the touched dofs";
    return false;
  }
  return true;
}

// Plain host entry (tests; no device): the basis of the dofs rel[0 .. n_c) (block-relative, ascending, closed under the box's operations) of a box of dims nodes
// x ndof dofs.  mult / dim: [10]; orb_size: [n_c] (the first *norb are set); orb_pos, row_irrep, row_index, row_partner: [n_c]; row_v: [3 n_c]; tables: [48 n_c],
// basis function `row` of an orbit of size s holds its s values at tables[48 row ...], in the order of the orbit's positions.
extern "C" int pmh_orbit_basis(const int *dims, int ndof, int n_c, const int *rel, int *norb, int *mult, int *dim, int *orb_size, int *orb_pos, int *row_irrep, int *row_index,
                               int *row_partner, double *row_v, double *tables)
{
  PMH_ARG(dims && ndof >= 1 && n_c >= 1 && rel && norb && mult && dim && orb_size && orb_pos && row_irrep && row_index && row_partner && row_v && tables);
  const long long nn = (long long)dims[0] * dims[1] * dims[2] * ndof;
  PMH_ARG(nn >= 1 && nn < (1LL << 31));
  const int                n = (int)nn;
  std::vector<int>         perm((size_t)48 * n), pos((size_t)n, -1), pm, ops(6 * 48);
  std::vector<signed char> sign((size_t)48 * n), sg;
  int                      nsym = 0;
  PMH_CHK(pmh_box_symmetries_ops(dims, ndof, nullptr, nullptr, nullptr, 0, &nsym, perm.data(), sign.data(), ops.data()));
  for (int i = 0; i < n_c; i++) {
    PMH_ARG(rel[i] >= 0 && rel[i] < n && (i == 0 || rel[i] > rel[i - 1]));
    pos[rel[i]] = i;
  }
  for (int g = 0; g < nsym; g++)
    for (int i = 0; i < n_c; i++) {
      const int t = pos[perm[(size_t)g * n + rel[i]]];
      if (t < 0) return pmh_set_error(PMH_ERR_ARG, "pmh_orbit_basis: the dofs are not closed under operation %d", g);
      pm.push_back(t), sg.push_back(sign[(size_t)g * n + rel[i]]);
    }
  oab_basis   b;
  std::string why;
  if (!oab_build(nsym, n_c, pm.data(), sg.data(), ops.data(), b, why)) return pmh_set_error(PMH_ERR_SUP, "pmh_orbit_basis: %s", why.c_str());
  *norb = b.norb;
  for (int i = 0; i < OAB_NIRREP; i++) mult[i] = b.m[i], dim[i] = b.d[i];
  memcpy(orb_size, b.osize.data(), sizeof(int) * (size_t)b.norb);
  memcpy(orb_pos, b.opos.data(), sizeof(int) * (size_t)n_c);
  memcpy(row_irrep, b.row_irrep.data(), sizeof(int) * (size_t)n_c);
  memcpy(row_index, b.row_index.data(), sizeof(int) * (size_t)n_c);
  memcpy(row_partner, b.row_partner.data(), sizeof(int) * (size_t)n_c);
  memcpy(row_v, b.row_v.data(), sizeof(double) * 3 * (size_t)n_c);
  memset(tables, 0, sizeof(double) * 48 * (size_t)n_c);
  for (int o = 0; o < b.norb; o++)
    for (int t = 0; t < b.osize[o]; t++) memcpy(tables + 48 * (size_t)(b.tbase[o] + t), b.tab.data() + b.toff[o] + (size_t)t * b.osize[o], sizeof(double) * (size_t)b.osize[o]);
  return PMH_SUCCESS;
}
