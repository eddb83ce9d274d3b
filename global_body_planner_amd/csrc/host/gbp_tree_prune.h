// gbp_tree_prune.h — a prune's remap (gbp_tree_prune_dev, include/gbp.h), a
// re-root's (gbp_tree_reroot_dev) or a graft's (gbp_tree_graft_dev) applied to
// the host copy of a tree.  Pure host code with no engine call.
#pragma once

#include <cstdint>
#include <vector>

#include "gbp_planner.h"

namespace gbp_amd {

// remap[n]: a vertex's new index or -1, as the device prune returns it — the
// kept vertices numbered 0, 1, ... in their order, the root kept as 0, a kept
// vertex's parent kept.  Moves the kept rows of v / a / parent / g (each of n
// rows; g may be null) to the front in place, parent as remap[parent], and
// returns how many there are; -1, with nothing changed, when remap is no such
// map for these parents.
int64_t applyPruneRemap(const int32_t *remap, int64_t n, State *v, Action *a, int32_t *parent,
                        double *g);

// tree k of a TreeDump (its four vectors shortened to the survivors)
bool applyPruneRemap(const std::vector<int32_t> &remap, TreeDump &trees, int k);

// What a trim by cost (gbp_tree_trim_host, include/gbp.h) did to a tree, counted
// from its remap and stage A's flags alone.
struct TrimRemapRecord {
  int64_t n_before = 0;     // vertices before the trim
  int64_t n_kept = 0;       // ... and after it
  int64_t n_flagged = 0;    // dropped: their own flag is 0 (over the bound or the budget)
  int64_t n_inherited = 0;  // dropped though their own flag is 1: an ancestor's is 0
};

// remap[n] as the device trim returns it (a prune's remap, see above) and
// keep[n], stage A's flags (gbp_tree_trim_flags_dev): a kept vertex has keep !=
// 0 and keep[0] != 0.  Tree k of `trees` is shortened to the survivors as
// applyPruneRemap does, g's rows moved as they are (a trim changes no g), and
// *rec (may be null) filled.  False, with nothing changed, when remap is no such
// map for these parents or keeps a vertex against its flag.
bool applyTrimRemap(const std::vector<int32_t> &remap, const std::vector<uint8_t> &keep, TreeDump &trees,
                    int k, TrimRemapRecord *rec = nullptr);

// remap[n] as the device re-root returns it: new_root numbered 0, the other
// kept vertices 1, 2, ... in ascending old index, a kept vertex other than
// new_root under a kept parent.  Moves the kept rows to the front in place:
// the new root first, its action zeroed and its parent -1, parent elsewhere as
// remap[parent].  g's rows (g may be null) are moved as they are: a re-root
// derives g again from the new root, and the caller takes it from the device
// tree.  Returns how many rows are kept; -1, with nothing changed, when remap
// is no such map for these parents.
int64_t applyRerootRemap(const int32_t *remap, int64_t n, int32_t new_root, State *v, Action *a,
                         int32_t *parent, double *g);

// tree k of a TreeDump (its four vectors shortened to the survivors)
bool applyRerootRemap(const std::vector<int32_t> &remap, int32_t new_root, TreeDump &trees, int k);

// remap[n] as the device graft returns it: the kept vertices numbered 1, 2, ...
// in ascending old index (0 is the new root state, no vertex of the tree),
// every attached vertex (attach[i] != 0) kept, every other kept vertex under a
// kept parent.  Tree k of `trees` becomes the root (its action zeroed, its
// parent -1, g 0) followed by the kept rows: an attached vertex under vertex 0
// by actions[i], the others under remap[parent] by their own action.  g's rows
// are moved as they are: a graft derives g again, and the caller takes it from
// the device tree.  False, with nothing changed, when remap is no such map for
// these parents and this attach.
bool applyGraftRemap(const std::vector<int32_t> &remap, const State &root,
                     const std::vector<uint8_t> &attach, const std::vector<Action> &actions,
                     TreeDump &trees, int k);

}  // namespace gbp_amd
