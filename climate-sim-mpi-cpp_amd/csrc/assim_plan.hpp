// assim_plan.hpp — the host mathematics of the ensemble analysis, without a device or the HIP headers (assim_plan.cpp):
// the plan that csim_ensemble_assimilate and the observation networks both build, its batches, and behind include/csim.h
// csim_ensemble_gc_table, csim_ensemble_assim_plan (the levels), csim_ensemble_perturb_taps and the host-only calls of
// the LETKF (csim_letkf_nodes, csim_letkf_blend, csim_letkf_plan).
// tools/assim_plan_host_check.cpp compiles it with plain g++ under AddressSanitizer.
#pragma once
#include <vector>

#include "obs_taps.hpp"

namespace csim {

// the (2 ly + 1) x (2 lx + 1) table of csim_ensemble_gc_table for half-widths it has returned
void gc_fill(double dx, double dy, double loc, int lx, int ly, double* table);

// Observations in the order the analysis takes them: by level, then input index.
struct AssimPlan {
    int nobs = 0, nlevels = 0, lx = 0, ly = 0;
    std::vector<int> off;      // level L holds the plan positions off[L] .. off[L + 1)
    std::vector<int> idx;      // the input index of every plan position
    std::vector<int> pi, pj;   // the cells in plan order
};
// The plan of nobs >= 0 observations at the cells (i, j) of an nx x ny grid with spacings dx, dy, after the checks
// of each observation in turn: inside the interior, y finite (where y is given), r finite and > 0.
int assim_plan_build(int nx, int ny, double dx, double dy, double loc, bool ordered, int nobs, const int* i,
                     const int* j, const double* r, const double* y, AssimPlan* p);

struct AssimBatch {
    int first, count;  // plan positions
    long wcells;       // the largest clipped window of the batch in cells
};
// the launches of a plan on an nx x ny grid: no batch crosses a level or holds more than `batch` observations
void assim_batches(int nx, int ny, const AssimPlan& p, int batch, std::vector<AssimBatch>* out);

// The lookup of the local analysis (csim_ensemble_assimilate_local): the interior cut into tiles of tile x tile cells
// (the last ones of a row or column clipped by the domain), ntx x nty of them, row-major.  Tile T holds
// pos[start[T] .. start[T + 1]): the plan positions of the observations whose window rectangle, clipped to the
// interior, meets the tile, sorted by input index.
struct LocalTiles {
    int tile = 0, ntx = 0, nty = 0;
    std::vector<int> start, pos;
};
// false: more than 2^31 - 1 entries (nothing is built)
bool local_tiles_build(int nx, int ny, const AssimPlan& p, int tile, LocalTiles* out);

// The lookup of the LETKF (csim_ensemble_assimilate_letkf) for the lattice of letkf_nodes.hpp with this spacing: node g
// = b nax + a holds pos[start[g] .. start[g + 1]): the plan positions of the observations whose window rectangle, clipped
// to the interior, contains the node's cell, sorted by input index.
struct LetkfLookup {
    int spacing = 0, nax = 0, nay = 0;
    std::vector<int> start, pos;
};
// false: more than 2^31 - 1 entries (nothing is built)
bool letkf_lookup_build(int nx, int ny, const AssimPlan& p, int spacing, LetkfLookup* out);

}  // namespace csim
