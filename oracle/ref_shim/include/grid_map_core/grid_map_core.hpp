/*
 * oracle/ref_shim/include/grid_map_core/grid_map_core.hpp -- TEST INFRASTRUCTURE ONLY.
 * Narrowed umbrella header: it comes first on the include path of oracle/_ref/libref_gridmap.so and
 * names only the grid_map_core headers whose sources that library compiles (GridMap, GridMapMath,
 * SubmapGeometry, BufferRegion and the GridMap / Submap / Line / Circle iterators).  Every other header
 * is still found in the reference's own include/ directory, which follows this one on the path.
 */
#pragma once

#include "grid_map_core/TypeDefs.hpp"
#include "grid_map_core/GridMap.hpp"
#include "grid_map_core/SubmapGeometry.hpp"
#include "grid_map_core/GridMapMath.hpp"
#include "grid_map_core/BufferRegion.hpp"
#include "grid_map_core/iterators/GridMapIterator.hpp"
#include "grid_map_core/iterators/SubmapIterator.hpp"
#include "grid_map_core/iterators/CircleIterator.hpp"
#include "grid_map_core/iterators/LineIterator.hpp"
