/*
 * STAND-IN for <ros/ros.h>, test infrastructure only.  The sources the parity
 * driver compiles include this header and use nothing from it.
 */
#ifndef GBP_STANDIN_ROS_H
#define GBP_STANDIN_ROS_H
#endif
