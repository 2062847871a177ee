// sort_probe.cpp -- TEST INFRASTRUCTURE ONLY: the genuine std::sort of the C++ library this file is compiled against, and an adversary
// for it.  oracle/strelka_oracle.c restates libstdc++'s std::sort (sko_sort_idx_by_key_desc) and the kernels restate it again; this
// file is what those restatements are compared with (tests/golden/make_sort_adversary.py, tests/test_germline_sort_adversary.py).
//
//   skp_std_sort_idx_by_key_desc   std::sort on an index array with comp(a, b) = key[a] > key[b], the comparator of
//                                  adjust_joint_eprob's sort_icall_by_eprob
//   skp_sort_adversary             an adversary in the manner of M. D. McIlroy, "A Killer Adversary for Quicksort" (Software -- Practice
//                                  and Experience 29(4), 1999): std::sort runs on 0..n-1 with a comparator that decides the items'
//                                  values only as the algorithm asks, always so that the pivot it has just picked turns out to be
//                                  an extreme element.  The values it ends with make the same std::sort take the same steps when
//                                  they are given up front: partitions that strip a few elements a time, until introsort's depth
//                                  limit runs out and the heap sort takes over.

#include <algorithm>
#include <cstdint>
#include <vector>

namespace
{

struct Adversary
{
    std::vector<int> val;
    int gas, nsolid, candidate;

    explicit Adversary(const int n) : val(n, n), gas(n), nsolid(0), candidate(0) {}

    // is item x less than item y?  Two undecided items: one of them (the likely pivot) is decided now, as the smallest value left
    bool less(const int x, const int y)
    {
        if (val[x] == gas && val[y] == gas) {
            if (x == candidate) val[x] = nsolid++;
            else val[y] = nsolid++;
        }
        if (val[x] == gas) candidate = x;
        else if (val[y] == gas) candidate = y;
        return val[x] < val[y];
    }
};

} // namespace

extern "C" {

void skp_std_sort_idx_by_key_desc(uint32_t* idx, const int n, const uint16_t* key)
{
    if (n <= 0) return;
    std::sort(idx, idx + n, [key](const uint32_t a, const uint32_t b) { return key[a] > key[b]; });
}

// val[n] <- a permutation of 0..n-1.
//   mirror == 0   std::sort ran with comp(a, b) = val[a] < val[b]: every pivot is a small element, the partitions' big part is the
//                 RIGHT one (the one __introsort_loop recurses into).  Keys that ask the same of comp(a, b) = key[a] > key[b]:
//                 key = base + (n - 1 - val) / k.
//   mirror != 0   std::sort ran with comp(a, b) = val[a] > val[b]: the big part is the LEFT one (the one __introsort_loop keeps
//                 looping on -- the chain a top-k selection follows).  Keys: key = base + val / k.
// Items the sort never had to decide get the values left over, in index order.
void skp_sort_adversary(const int n, const int mirror, int32_t* val)
{
    if (n <= 0) return;
    Adversary adv(n);
    std::vector<uint32_t> idx(n);
    for (int i = 0; i < n; ++i) idx[i] = uint32_t(i);
    if (mirror) std::sort(idx.begin(), idx.end(), [&adv](const uint32_t a, const uint32_t b) { return adv.less(int(b), int(a)); });
    else std::sort(idx.begin(), idx.end(), [&adv](const uint32_t a, const uint32_t b) { return adv.less(int(a), int(b)); });
    for (int i = 0; i < n; ++i) {
        if (adv.val[i] == adv.gas) adv.val[i] = adv.nsolid++;
        val[i] = adv.val[i];
    }
}

} // extern "C"
