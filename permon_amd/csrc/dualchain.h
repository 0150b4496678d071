// Fused dual-space chain of the penalised, projected FETI operator (dualchain.hip; internal)
#pragma once
#include "pmh_internal.h"

struct pmh_dualchain_s;
typedef pmh_dualchain_s *pmh_dualchain;

// F must offer pmh_op_s::stages; PMH_EPI_UNSUPPORTED (no error recorded) where the chain does not apply
int  pmh_dc_create(pmh_qppf pf, pmh_op F, pmh_dualchain *out);
void pmh_dc_destroy(pmh_dualchain dc);
// y = rho Q x + P F P x (+ the vector phase of epi in the last kernel); epi may be nullptr
int  pmh_dc_apply(pmh_dualchain dc, const double *x, double *y, double rho, const pmh_vec_epi *epi);
int  pmh_dc_emit_begin(pmh_dualchain dc, const double *x, const double *p, pmh_emit_args *ea);
// x or p are about to change without emission; keep_applied: the vector the chain was last applied to is not among them (its intermediates stay on record)
void pmh_dc_invalidate(pmh_dualchain dc, bool keep_applied = false);
// pmh_dc_apply for a caller who asserts that x still holds what the chain was last applied to: the last kernel alone on the intermediates the chain kept, where its
// own record (address, no pmh_free since, the same stages of F) agrees -- the bits of the full application; the full application otherwise.  *replayed (may be
// nullptr) = 1 where the last kernel ran alone, 0 where the full application did
int  pmh_dc_replay(pmh_dualchain dc, const double *x, double *y, double rho, const pmh_vec_epi *epi, int *replayed);
// test entries: a kernel that writes x and emits G0 x (x as it is); the segment sums of G0 p the last gradient split emitted
int  pmh_dc_test_emit(pmh_dualchain dc, const double *x);
int  pmh_dc_test_direction_sums(pmh_dualchain dc, int cap, double *host, int *nseg);
// SMALXE's ||B u||: every emission of the iterate also leaves T G0 u in Gu (m doubles) and its squared norm in d_scal / h_scal[slot]
int  pmh_dc_set_norm_target(pmh_dualchain dc, double *Gu, int slot);
bool pmh_dc_norm_ready(pmh_dualchain dc, const double *u);
// launches of the last application (tests, bench)
int  pmh_dc_last_launches(pmh_dualchain dc);
// test entries: what the chain planned; what one application left behind (see dualchain.hip)
int  pmh_dc_test_info(pmh_dualchain dc, long long info[10]);
int  pmh_dc_test_read(pmh_dualchain dc, int what, int cap, double *host, int *len);
