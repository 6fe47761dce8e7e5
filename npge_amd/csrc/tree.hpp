// Host-only tree building: TreeNode::neighbor_joining, upgma,
// clone_with_pseudo_leafs, all_descendants and print_newick
// (src/util/tree.cpp:65-82, 93-98, 188-258, 285-480) restated over node
// numbers instead of pointers.  Nothing here touches HIP.
//
// Conventions (DESIGN.md "Determinism conventions"): nodes are numbered in
// creation order -- the leaves 0 .. n-1 in the order they are added, then each
// internal node as it is made; the root has no number (parent -1 = the root);
// make_pair(a, b) is (lower number, higher number) where the reference takes
// the lower address; find_min_pair keeps the first minimum in its (i, j) loop
// order over the current node list, whose survivors keep their order with the
// new node appended.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace npgx {
namespace tree {

enum ShowBootstrap { NO_BOOTSTRAP = 0, BOOTSTRAP_IN_BRACES = 1, BOOTSTRAP_BEFORE_LENGTH = 2 };

struct Node {
    int32_t parent = -1;  // -1: the root
    int32_t leaf = -1;    // a leaf's index (>= 0); -2 - index: its pseudo leaf ".name"; -1: an internal node
    double length = 0.0;
    double bootstrap = 0.0;
    std::vector<int32_t> children;
};

struct Tree {
    std::vector<Node> nodes;
    std::vector<int32_t> top;  // the root's children
    double root_bootstrap = 0.0;
};

// one entry of a tree in print order (the root first, then all_descendants)
struct TableNode {
    int32_t parent;  // entry of the parent; -1: the root
    int32_t leaf;    // as Node::leaf
    double length, bootstrap;
};

// a tree of n leaves under the root
Tree make_leaves(int32_t n);
// d: n x n distances between the leaves (row-major, symmetric, zero diagonal)
void neighbor_joining(Tree& t, const std::vector<double>& d);
void upgma(Tree& t, const std::vector<double>& d);
Tree clone_with_pseudo_leafs(const Tree& t);
// all_descendants of the root: every node, parents before children
void descendants(const Tree& t, std::vector<int32_t>& out);
// the leaf indices under node k (k itself when it is a leaf)
void leaves_under(const Tree& t, int32_t k, std::vector<int32_t>& out);
std::vector<TableNode> table(const Tree& t);
// newick(lengthes, sbs) (tree.cpp:188-258); names[i] = leaf i's name
std::string newick(const Tree& t, const std::vector<std::string>& names, bool lengthes, ShowBootstrap sbs);
// ostream << double at the default precision
std::string format_double(double x);
// FragmentDistance::fragment_distance's penalty (FragmentDistance.cpp:31-69)
// of two gapped rows of L columns, one column after another on the host (the
// CPU yardstick of k_pair_dist): the columns c in [1, L - 2] that differ while
// c - 1 and c + 1 are equal and no gap
int64_t fragment_penalty(const char* a, const char* b, int64_t L);

}  // namespace tree
}  // namespace npgx
