/*
 * oracle/ref_shim/include/rna_ref_rand.h -- TEST INFRASTRUCTURE ONLY.  Force-included (-include) into the
 * reference's rrt_planner.cpp by oracle/Makefile: its rand() calls go to rna_ref_rand() in
 * ref_gridmap_shim.cpp, which returns this libc's rand() and only counts the calls (see there).  The
 * standard headers come first so that the macro renames nothing of theirs.
 */
#pragma once
#include <Eigen/Core>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <map>
#include <memory>
#include <unordered_map>

extern "C" int rna_ref_rand();
#define rand rna_ref_rand
