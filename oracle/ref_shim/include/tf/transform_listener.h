/*
 * oracle/ref_shim/include/tf/transform_listener.h -- TEST INFRASTRUCTURE ONLY.  Declares the one name
 * that move_control's MapUpdater constructor takes (tf::TransformListener&); nothing of tf is used.
 */
#pragma once

namespace tf {
class TransformListener {};
}  // namespace tf
