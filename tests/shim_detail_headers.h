// every header of shim/qn_map, for the two translation units of tests/shim_detail.cpp (tests/test_shim_detail.py checks that none is missing)
#pragma once
#include <qn_map/corrected_map.hpp>
#include <qn_map/detail.hpp>
#include <qn_map/freespace.hpp>
#include <qn_map/loop_submaps.hpp>
#include <qn_map/map_clusters.hpp>
#include <qn_map/map_distance.hpp>
#include <qn_map/map_frontier.hpp>
#include <qn_map/map_ground.hpp>
#include <qn_map/map_localize.hpp>
#include <qn_map/map_normals.hpp>
#include <qn_map/map_occupancy.hpp>
#include <qn_map/map_outliers.hpp>
#include <qn_map/map_route.hpp>
#include <qn_map/map_view.hpp>
#include <qn_map/scan_context.hpp>
#include <qn_map/static_map.hpp>
