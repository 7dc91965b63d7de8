// Internal (non-exported) host helpers shared by the C-ABI translation units.
#pragma once
#include <string>

#include "prl_defs.h"
#include "prl_tree.h"

void prl_set_error(const std::string& msg);
extern "C" const PrlFlatTree* prl_tree_flat(const prl_tree_t* tree);

// The tree handle behind prl_tree_t. `obs`: the device side of the public-tree observations (prl_tree_obs.hip) -- the env state of every
// node in HBM and the per-call scratch --, made on first use, freed with the tree.
struct PrlTreeObs;
void prl_tree_obs_free(PrlTreeObs* obs);
struct prl_tree {
    PrlFlatTree t;
    mutable PrlTreeObs* obs = nullptr;
};
