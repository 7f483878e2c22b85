/*
 * oracle/ref_shim/include/ros/ros.h -- TEST INFRASTRUCTURE ONLY.  Declares the one name that
 * move_control's MapUpdater constructor takes (ros::NodeHandle&); nothing of ROS is used.
 */
#pragma once

namespace ros {
class NodeHandle {};
}  // namespace ros
