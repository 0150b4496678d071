// The set-up loop of the explicit local dual operators, written once (fx_assemble_run, fexplicit.hip) for the five storage forms of fexplicit.hip / fshared.hip.
// The loop owns the solver (pmh_asm_solver), the sorting of slots into classes and their size checks, the window of batches, the buffers and the solver's
// tolerances (a scope guard: every way out frees and restores), the unit entries, the solve, its iteration-limit test, the launch check, the progress report and
// the timing.  A storage form hands it a plan, decided once per call:
//   todo[c]    the columns to solve for class c, in order: the relative dof of the unit entry and the form's own row id for what comes back.  Column j goes to the
//              class's slot j % (its slots) in batch j / (its slots); idle slots solve nothing.
//   write      (class, row id, solution of the slot) -> the form's store launches
//   check[c]   optional: the rows of class c that the form filled by symmetry.  The loop solves min(their number, the class's slots) of them, spread over the list,
//              directly in ONE batch after the others (batch number nbatch - 1 of fx_batch_window)
//   check_row  (class, row id, solution, d_out) -> the form's check launch: per workgroup the largest |stored - solved| and the largest |solved| of the row as a
//              pair in d_out (room for 64 pairs); returns the number of pairs.  The bound and the error are the loop's.
#pragma once
#include <functional>
#include <vector>

#include "feti_internal.h"

struct fx_asm_row {
  int rel, id;
};
struct fx_asm_plan {
  std::vector<int>                     nloc; // rows of the class's blocks (what its slots must have); -1: the operator has nothing of the class, it needs no slot
  std::vector<std::vector<fx_asm_row>> todo, check;
  std::function<void(int, int, const double *)>          write;
  std::function<int(int, int, const double *, double *)> check_row;
  explicit fx_asm_plan(int ncls) : nloc(ncls, -1), todo(ncls), check(ncls) {}
};
// slot_class[s]: class of the matrix in slot s (values outside the plan's classes: the slot idles); *n_solves grows by the columns solved; w: feti_internal.h
int fx_assemble_run(pmh_ctx ctx, const fx_asm_plan &P, pmh_matinv solver, int nslots, const int *slot_class, double rtol, int max_it, long long *n_solves, fx_batch_window *w);
// wrow[i] = u[rel[i]], i < n: a row of W stored in full from a solution (row p = column p, K^+ symmetric)
void fx_extract_row(pmh_ctx ctx, int n, const int *rel, const double *u, double *wrow);
