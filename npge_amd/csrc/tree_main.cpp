// Stand-alone driver of the host tree code (tree.cpp), for tests and CPU
// timing; it is not part of the library.  Standard input holds any number of
// cases:
//   tree METHOD SBS PSEUDO N   then N x N distances (any strtod form)
//       METHOD nj | upgma; SBS 0 no, 1 in-braces, 2 before-length; PSEUDO 0 | 1.
//       The leaves are named n0, n1, ...  Prints "nodes K", K lines
//       "parent leaf length bootstrap" (the doubles as %a), "text B" and the
//       B bytes of newick text followed by a newline.
//   pairs N L REPEAT           then N rows of L characters, one per line
//       fragment_penalty of every pair (i < j), REPEAT times on one thread.
//       Prints "pairs P", the P penalties on one line, "ms T" (the median run).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "tree.hpp"

using namespace npgx::tree;

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "tree") {
            std::string method;
            int sbs = 0, pseudo = 0, n = 0;
            if (!(std::cin >> method >> sbs >> pseudo >> n) || n < 0 || sbs < 0 || sbs > 2) return 2;
            std::vector<double> d((size_t)n * (size_t)n);
            for (double& x : d) {
                std::string tok;
                if (!(std::cin >> tok)) return 2;
                x = strtod(tok.c_str(), nullptr);
            }
            Tree t = make_leaves(n);
            if (method == "nj")
                neighbor_joining(t, d);
            else if (method == "upgma")
                upgma(t, d);
            else
                return 2;
            if (pseudo) t = clone_with_pseudo_leafs(t);
            std::vector<std::string> names;
            for (int i = 0; i < n; i++) names.push_back("n" + std::to_string(i));
            const std::vector<TableNode> tb = table(t);
            printf("nodes %zu\n", tb.size());
            for (const TableNode& x : tb) printf("%d %d %a %a\n", x.parent, x.leaf, x.length, x.bootstrap);
            const std::string text = newick(t, names, true, (ShowBootstrap)sbs);
            printf("text %zu\n%s\n", text.size(), text.c_str());
        } else if (what == "pairs") {
            long n = 0, L = 0, repeat = 1;
            if (!(std::cin >> n >> L >> repeat) || n < 0 || L < 0 || repeat < 1) return 2;
            std::vector<std::string> rows((size_t)n);
            for (std::string& r : rows) {
                if (L > 0 && !(std::cin >> r)) return 2;
                if ((long)r.size() != L) return 2;
            }
            std::vector<int64_t> pen;
            std::vector<double> ms;
            for (long rep = 0; rep < repeat; rep++) {
                pen.clear();
                const auto t0 = std::chrono::steady_clock::now();
                for (long i = 0; i < n; i++)
                    for (long j = i + 1; j < n; j++)
                        pen.push_back(fragment_penalty(rows[(size_t)i].data(), rows[(size_t)j].data(), L));
                ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            printf("pairs %zu\n", pen.size());
            for (int64_t p : pen) printf("%lld ", (long long)p);
            printf("\nms %.6f\n", ms[ms.size() / 2]);
        } else {
            return 2;
        }
    }
    return 0;
}
