// Host-only tree building (tree.hpp).  The arithmetic restates
// src/util/tree.cpp literally, in the reference's order of operations; this
// file is compiled with -ffp-contract=off so that no multiply-add is fused.
#include "tree.hpp"

#include <cstdio>
#include <stdexcept>

namespace npgx {
namespace tree {

namespace {

// the reference's std::map<Pair, double> over the numbered nodes: a square
// matrix, an absent entry reads 0.0 as operator[] gives (d(x, x) included)
struct Distances {
    int32_t m;
    std::vector<double> v;
    explicit Distances(int32_t m_) : m(m_), v((size_t)m_ * (size_t)m_, 0.0) {}
    double get(int32_t a, int32_t b) const { return v[(size_t)a * m + b]; }
    void set(int32_t a, int32_t b, double x) {
        v[(size_t)a * m + b] = x;
        v[(size_t)b * m + a] = x;
    }
};

struct Pair {
    int32_t first = -1, second = -1;
};

// make_pair (tree.cpp:263-269): the lower number first
Pair make_pair(int32_t a, int32_t b) {
    Pair p;
    p.first = a < b ? a : b;
    p.second = a < b ? b : a;
    return p;
}

// tree.cpp:285-294
Distances build_distances(int32_t n, const std::vector<double>& d) {
    Distances dist(2 * n + 1);
    for (int32_t i = 0; i < n; i++)
        for (int32_t j = i + 1; j < n; j++) dist.set(i, j, d[(size_t)i * n + j]);
    return dist;
}

// tree.cpp:296-309: the first minimum in (i, j) order
Pair find_min_pair(const Distances& distances, const std::vector<int32_t>& nodes) {
    Pair min_pair;
    for (size_t i = 0; i < nodes.size(); i++)
        for (size_t j = i + 1; j < nodes.size(); j++) {
            const double distance = distances.get(nodes[i], nodes[j]);
            if (min_pair.first < 0 || distance < distances.get(min_pair.first, min_pair.second))
                min_pair = make_pair(nodes[i], nodes[j]);
        }
    return min_pair;
}

// a new internal node under the root with the pair's nodes as its children
int32_t join(Tree& t, const Pair& p) {
    const int32_t k = (int32_t)t.nodes.size();
    t.nodes.emplace_back();
    t.nodes[(size_t)k].children = {p.first, p.second};
    t.nodes[(size_t)p.first].parent = k;
    t.nodes[(size_t)p.second].parent = k;
    return k;
}

void replace_pair(std::vector<int32_t>& nodes, const Pair& p, int32_t k) {
    std::vector<int32_t> left;
    for (int32_t x : nodes)
        if (x != p.first && x != p.second) left.push_back(x);
    left.push_back(k);
    nodes.swap(left);
}

// tree.cpp:311-339
void upgma_round(Tree& t, Distances& distances, std::vector<int32_t>& nodes) {
    const Pair min_pair = find_min_pair(distances, nodes);
    if (min_pair.first < 0) throw std::runtime_error("No branch for upgma round");
    const double min_distance = distances.get(min_pair.first, min_pair.second);
    const int32_t new_node = join(t, min_pair);
    t.nodes[(size_t)min_pair.first].length = min_distance / 2.0;
    t.nodes[(size_t)min_pair.second].length = min_distance / 2.0;
    for (int32_t node_i : nodes)
        if (node_i != min_pair.first && node_i != min_pair.second) {
            const double d1 = distances.get(node_i, min_pair.first);
            const double d2 = distances.get(node_i, min_pair.second);
            distances.set(node_i, new_node, 0.5 * d1 + 0.5 * d2);
        }
    replace_pair(nodes, min_pair, new_node);
}

// tree.cpp:360-375: d(i, k) and d(j, k) leave for every k, k = i and k = j included
void calculate_q(Distances& Q, const Distances& distances, const std::vector<int32_t>& nodes) {
    for (size_t i = 0; i < nodes.size(); i++)
        for (size_t j = i + 1; j < nodes.size(); j++) {
            double distance = ((double)nodes.size() - 2.0) * distances.get(nodes[i], nodes[j]);
            for (size_t k = 0; k < nodes.size(); k++) {
                distance -= distances.get(nodes[i], nodes[k]);
                distance -= distances.get(nodes[j], nodes[k]);
            }
            Q.set(nodes[i], nodes[j], distance);
        }
}

// tree.cpp:377-403
double distance_to_first(const Pair& min_pair, const Distances& distances, const std::vector<int32_t>& nodes) {
    const double min_distance = distances.get(min_pair.first, min_pair.second);
    double s = 0;
    for (int32_t node_k : nodes)
        if (node_k != min_pair.first && node_k != min_pair.second) {
            s += distances.get(min_pair.first, node_k);
            s -= distances.get(min_pair.second, node_k);
        }
    double dist;
    if (nodes.size() > 2)
        dist = 0.5 * min_distance + 0.5 * s / (double)(nodes.size() - 2);
    else
        dist = 0.5 * min_distance;
    if (dist < 0.0) dist = 0.0;
    if (dist > min_distance) dist = min_distance;
    return dist;
}

// tree.cpp:405-411
double distance_to_pair(const Pair& min_pair, const Distances& distances, int32_t node_k) {
    const double min_distance = distances.get(min_pair.first, min_pair.second);
    const double dist_f = distances.get(min_pair.first, node_k);
    const double dist_s = distances.get(min_pair.second, node_k);
    return 0.5 * (dist_f + dist_s - min_distance);
}

// tree.cpp:413-444
void neighbor_joining_round(Tree& t, Distances& distances, std::vector<int32_t>& nodes) {
    Distances Q(distances.m);
    calculate_q(Q, distances, nodes);
    const Pair min_pair = find_min_pair(Q, nodes);
    if (min_pair.first < 0) throw std::runtime_error("No min element of Q for neighbor joining");
    const int32_t new_node = join(t, min_pair);
    const double min_distance = distances.get(min_pair.first, min_pair.second);
    const double distance_to_left = distance_to_first(min_pair, distances, nodes);
    const double distance_to_right = min_distance - distance_to_left;
    t.nodes[(size_t)min_pair.first].length = distance_to_left;
    t.nodes[(size_t)min_pair.second].length = distance_to_right;
    for (int32_t node_k : nodes)
        if (node_k != min_pair.first && node_k != min_pair.second)
            distances.set(new_node, node_k, distance_to_pair(min_pair, distances, node_k));
    replace_pair(nodes, min_pair, new_node);
}

void check_matrix(const Tree& t, const std::vector<double>& d) {
    const size_t n = t.nodes.size();
    if (t.top.size() != n || d.size() != n * n) throw std::runtime_error("tree: the matrix does not fit the leaves");
}

void descend(const Tree& t, int32_t k, std::vector<int32_t>& out) {
    out.push_back(k);
    for (int32_t c : t.nodes[(size_t)k].children) descend(t, c, out);
}

int32_t clone_pseudo(const Tree& t, int32_t k, Tree& out, int32_t parent) {
    const Node& src = t.nodes[(size_t)k];
    const int32_t me = (int32_t)out.nodes.size();
    out.nodes.emplace_back();
    out.nodes[(size_t)me].parent = parent;
    out.nodes[(size_t)me].length = src.length;
    out.nodes[(size_t)me].bootstrap = src.bootstrap;
    std::vector<int32_t> ch;
    if (src.leaf >= 0) {
        for (int32_t v : {src.leaf, -2 - src.leaf}) {  // the leaf's clone (length 0, bootstrap 0), then ".name"
            ch.push_back((int32_t)out.nodes.size());
            out.nodes.emplace_back();
            out.nodes.back().parent = me;
            out.nodes.back().leaf = v;
        }
    } else {
        for (int32_t c : src.children) ch.push_back(clone_pseudo(t, c, out, me));
    }
    out.nodes[(size_t)me].children = ch;
    return me;
}

void print_node(const Tree& t, int32_t k, int depth, const std::vector<std::string>& names, bool lengthes,
                ShowBootstrap sbs, std::string& o) {
    // k = -1: the root (no parent: neither bootstrap nor length before the braces)
    const bool root = k < 0;
    const int32_t leaf = root ? -1 : t.nodes[(size_t)k].leaf;
    const double length = root ? 0.0 : t.nodes[(size_t)k].length;
    const double bootstrap = root ? t.root_bootstrap : t.nodes[(size_t)k].bootstrap;
    if (leaf != -1) {  // LeafNode::print_newick_impl (tree.cpp:249-258)
        if (leaf >= 0)
            o += names[(size_t)leaf];
        else
            o += "." + names[(size_t)(-2 - leaf)];
        if (lengthes) o += ":" + format_double(length);
    } else {  // TreeNode::print_newick_impl (tree.cpp:201-231)
        const std::string indent((size_t)depth * 2, ' ');
        o += '(';
        bool first = true;
        for (int32_t c : root ? t.top : t.nodes[(size_t)k].children) {
            if (!first) o += ',';
            first = false;
            o += '\n' + indent + "  ";
            print_node(t, c, depth + 1, names, lengthes, sbs, o);
        }
        o += "\n" + indent + ')';
        if (lengthes && !root) {
            if (sbs == BOOTSTRAP_BEFORE_LENGTH) o += format_double(bootstrap);
            o += ":" + format_double(length);
        }
    }
    if (sbs == BOOTSTRAP_IN_BRACES) o += "[" + format_double(bootstrap) + "]";
}

}  // namespace

std::string format_double(double x) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%g", x);
    return buf;
}

int64_t fragment_penalty(const char* a, const char* b, int64_t L) {
    int64_t penalty = 0;
    for (int64_t c = 1; c + 1 < L; c++) {
        const bool prev_good = a[c - 1] == b[c - 1] && a[c - 1] != '-';
        const bool curr_good = a[c] != b[c];
        const bool next_good = a[c + 1] == b[c + 1] && a[c + 1] != '-';
        penalty += prev_good && curr_good && next_good;
    }
    return penalty;
}

Tree make_leaves(int32_t n) {
    Tree t;
    t.nodes.resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        t.nodes[(size_t)i].leaf = i;
        t.top.push_back(i);
    }
    return t;
}

// TreeNode::upgma (tree.cpp:341-358)
void upgma(Tree& t, const std::vector<double>& d) {
    check_matrix(t, d);
    const int32_t n = (int32_t)t.nodes.size();
    if (n == 0) throw std::runtime_error("upgma: no leaves");
    Distances distances = build_distances(n, d);
    std::vector<int32_t> nodes = t.top;
    for (int32_t round = 0; round < n - 1; round++) upgma_round(t, distances, nodes);
    t.top = nodes;
}

// TreeNode::neighbor_joining (tree.cpp:446-480)
void neighbor_joining(Tree& t, const std::vector<double>& d) {
    check_matrix(t, d);
    const int32_t n = (int32_t)t.nodes.size();
    Distances distances = build_distances(n, d);
    std::vector<int32_t> nodes = t.top;
    if (n <= 1) return;
    if (n == 2) {
        const double d01 = distances.get(nodes[0], nodes[1]);
        t.nodes[(size_t)nodes[0]].length = d01 / 2.0;
        t.nodes[(size_t)nodes[1]].length = d01 / 2.0;
        return;
    }
    for (int32_t round = 0; round < n - 3; round++) neighbor_joining_round(t, distances, nodes);
    const Pair pair01 = make_pair(nodes[0], nodes[1]);
    const double l0 = distance_to_first(pair01, distances, nodes);
    const double l1 = distances.get(pair01.first, pair01.second) - l0;
    const double l2 = distance_to_pair(pair01, distances, nodes[2]);
    t.nodes[(size_t)pair01.first].length = l0;
    t.nodes[(size_t)pair01.second].length = l1;
    t.nodes[(size_t)nodes[2]].length = l2;
    t.top = nodes;
}

// TreeNode::clone_with_pseudo_leafs (tree.cpp:65-82)
Tree clone_with_pseudo_leafs(const Tree& t) {
    Tree out;
    out.root_bootstrap = t.root_bootstrap;
    for (int32_t c : t.top) out.top.push_back(clone_pseudo(t, c, out, -1));
    return out;
}

// TreeNode::all_descendants (tree.cpp:93-98)
void descendants(const Tree& t, std::vector<int32_t>& out) {
    for (int32_t c : t.top) descend(t, c, out);
}

void leaves_under(const Tree& t, int32_t k, std::vector<int32_t>& out) {
    std::vector<int32_t> all;
    descend(t, k, all);
    for (int32_t x : all)
        if (t.nodes[(size_t)x].leaf >= 0) out.push_back(t.nodes[(size_t)x].leaf);
}

std::vector<TableNode> table(const Tree& t) {
    std::vector<int32_t> order;
    descendants(t, order);
    std::vector<int32_t> entry(t.nodes.size(), -1);
    for (size_t i = 0; i < order.size(); i++) entry[(size_t)order[i]] = (int32_t)i + 1;
    std::vector<TableNode> out;
    out.push_back(TableNode{-1, -1, 0.0, t.root_bootstrap});
    for (int32_t k : order) {
        const Node& nd = t.nodes[(size_t)k];
        out.push_back(TableNode{nd.parent < 0 ? 0 : entry[(size_t)nd.parent], nd.leaf, nd.length, nd.bootstrap});
    }
    return out;
}

// TreeNode::newick (tree.cpp:188-199)
std::string newick(const Tree& t, const std::vector<std::string>& names, bool lengthes, ShowBootstrap sbs) {
    std::string o;
    print_node(t, -1, 0, names, lengthes, sbs, o);
    o += ';';
    return o;
}

}  // namespace tree
}  // namespace npgx
