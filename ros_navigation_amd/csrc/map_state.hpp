// map_state.hpp -- what the next compose or search has to redo, and every way that changes.  Plain C++ (no HIP): the rule
// is checked on the CPU against tests/_mapmodel.py's statement of it (tests/cpp/map_state_test.cpp).
#pragma once

#include "../../include/rna.h"

namespace rna {

// rna_compose_master in three answers (MapState::plan_compose); the enqueues follow them in this order
enum class ComposeCopy { Whole, DirtyTiles, Fused };   // master = laser: the layer, the flagged tiles, or compose_nbr_tiles_kernel (copy + masks + flags at once)
enum class ComposeMasks { AlreadyWaiting, MarkWaiting, RingRefresh, FootprintRefresh };
enum class ComposeLastDirty { AllOnes, CopyOfFlags, ArraysSwap };   // what rna_last_dirty_tiles reads afterwards
struct ComposePlan { ComposeCopy copy; ComposeMasks masks; ComposeLastDirty last_dirty; };

class MapState {
 public:
  // counts the calls that can change the neighbour masks (map updates, compose, uploads / fills / unpacks, moves, a new
  // robot radius), whether or not they did: a goal field, clearance field or frontier set built at another count is stale
  unsigned long long epoch = 0;

  bool masks_waiting() const { return masks_waiting_; }

  // a layer was written with no record of where: upload, fill, a device pointer handed out, an untracked unpack,
  // fromOccupancyGrid, HIMM on the master or the range layer
  void layer_written(int layer) {
    ++epoch;
    // the master no longer equals the laser outside the dirty tiles, so the next compose has to be the reference's
    // whole-layer copy (map_provider.cpp:221); so it has when the laser changed under the flags
    if (layer == RNA_LAYER_MASTER) masks_waiting_ = master_written_ = true;
    if (layer == RNA_LAYER_LASER) laser_replaced_ = true;
  }
  // tiles of a layer were written and flagged in dirty_tiles: HIMM on the laser, the tracked unpacks
  void tiles_written() { ++epoch; }
  // rna_move; the masks are stored per buffer cell and adjacency is in map space, so a shift of a cell or more unsettles them
  void moved(bool by_a_cell) { ++epoch; masks_waiting_ |= by_a_cell; }
  void radius_set() { ++epoch; masks_waiting_ = true; }
  void masks_rebuilt() { masks_waiting_ = false; }   // map_prepare_nbr
  // this engine is a clone or a submap: its layers were just filled from the parent's
  void cloned() { masks_waiting_ = laser_replaced_ = true; }

  void compose_begins() { ++epoch; }
  ComposePlan plan_compose(int mode, bool buffer_moved, bool has_radius) const {
    const bool replaced = laser_replaced_ || master_written_;
    // the usual case of the replan loop: dirty tiles only, masks valid before -- one launch
    if (mode == 0 && !replaced && !buffer_moved && !masks_waiting_ && !has_radius)
      return {ComposeCopy::Fused, ComposeMasks::RingRefresh, ComposeLastDirty::ArraysSwap};
    const bool whole = mode == 1 || replaced;
    // a layer was replaced: nothing is known about which masks are still valid; moved buffer: dirty tiles (buffer space)
    // do not line up with mask tiles (map space).  Masks valid before: only the dirty tiles and their ring change, through
    // footprint.hip with a radius (a changed tile reaches r / res <= 63 cells, inside its ring)
    const ComposeMasks masks = (replaced || buffer_moved) ? ComposeMasks::MarkWaiting
                               : masks_waiting_           ? ComposeMasks::AlreadyWaiting
                               : has_radius               ? ComposeMasks::FootprintRefresh
                                                          : ComposeMasks::RingRefresh;
    return {whole ? ComposeCopy::Whole : ComposeCopy::DirtyTiles, masks, whole ? ComposeLastDirty::AllOnes : ComposeLastDirty::CopyOfFlags};
  }
  void composed(const ComposePlan& plan) {
    if (plan.masks == ComposeMasks::MarkWaiting) masks_waiting_ = true;
    laser_replaced_ = master_written_ = false;
  }

 private:
  bool laser_replaced_ = false;   // the laser was replaced wholesale: its dirty flags do not cover the change
  bool master_written_ = false;   // the master was written directly: it differs from the laser outside the dirty tiles
  bool masks_waiting_ = true;     // the neighbour masks wait for a rebuild from the master (map_prepare_nbr)
};

}  // namespace rna
