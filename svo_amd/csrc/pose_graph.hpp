// Pose-graph optimisation on the device (pose_graph.hip): one workgroup runs the
// whole Levenberg-Marquardt of one problem, its conjugate gradients included, in
// one launch.
#pragma once

#include "common.hpp"
#include "pose_graph_model.hpp"

namespace svo {

// Problem p: nodes [p*max_nodes, + n_nodes[p]) of poses_in / fixed, edges
// [p*max_edges, + n_edges[p]) of edge_ij (pairs i, j within the problem), edge_Z
// (12) and edge_info (21); a null count array means the maximum. The incidence
// lists are the host's (pose_graph_api.cpp, incidence_lists): node n of problem p
// owns inc_list[p*2*max_edges + inc_start[p*(max_nodes+1) + n] ..
// inc_start[.. + n + 1]), each entry 2*edge + end (end 0: the node is the edge's
// i), ascending. poses_out may be poses_in. The scratch arrays are carved per
// batch, their sizes below in doubles; nothing in them survives a launch.
struct PoseGraphBatch {
    int P = 0, max_nodes = 0, max_edges = 0;
    const int *n_nodes = nullptr, *n_edges = nullptr;
    const double* poses_in = nullptr;
    double* poses_out = nullptr;
    const uint8_t* fixed = nullptr;
    const int* edge_ij = nullptr;
    const double* edge_Z = nullptr;
    const double* edge_info = nullptr;
    const int* inc_start = nullptr;
    const int* inc_list = nullptr;
    double delta = 0;
    int max_iterations = 0, max_cg = 0;
    // scratch
    double* cur = nullptr;    // P*max_nodes*12: the current poses
    double* trial = nullptr;  // P*max_nodes*12
    double* terms = nullptr;  // P*kPgEdgeTerms*max_edges: term k of edge e at [k*max_edges + e]
    double* node = nullptr;   // P*27*max_nodes: sum k of node n at [k*max_nodes + n]
    double* chol = nullptr;   // P*21*max_nodes: the preconditioner's factors, likewise
    // results
    double* costs = nullptr;       // [P][2], required
    int* iterations = nullptr;     // [P], required
    int* cg_iterations = nullptr;  // [P], required: A p products over the whole run
    // the test view, each nullable: written by the first linearisation
    double* lin_e = nullptr;     // [P][max_edges][6]
    double* lin_w = nullptr;     // [P][max_edges]
    double* lin_Ji = nullptr;    // [P][max_edges][36]
    double* lin_Jj = nullptr;    // [P][max_edges][36]
    double* lin_node = nullptr;  // [P][max_nodes][27]
};
// hipErrorInvalidValue (nothing launched): sizes outside 0 .. SVO_PG_MAX_NODES /
// SVO_PG_MAX_EDGES, max_iterations outside 0 .. SVO_PG_MAX_ITERATIONS, max_cg
// outside 1 .. SVO_PG_MAX_CG, a required pointer null.
hipError_t launch_pose_graph(const PoseGraphBatch& b, hipStream_t st);

}  // namespace svo
