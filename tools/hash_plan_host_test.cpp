// Host dump of csrc/hash_plan.h for tests/test_hash_schedules.py and
// tests/test_tree_top_schedule.py.  Build: g++ -std=c++20 -I celestia-app_amd/csrc.
//
//   hash_plan_host_test [NAME=VALUE ...]
//     P k n parts p i0 m stop room : launch launch ...
//       the plan of part p of every (k, n): k in 1, 2, 4 .. 1024, n in 1 .. 1024
//       (<= 64 at k = 256, <= 32 at k = 512, <= 8 at k = 1024: in-place arenas
//       of 16 GiB).  A launch is
//       kernel,n_in,sub,wide,lv,n_dig,pair,ragged,pmax,mode,threads,persistent,scratch
//       (hash_plan.h PlanLaunch; sub is tpw for the tree top).
//   hash_plan_host_test --top [NAME=VALUE ...]
//     T W n top_wide top wide
//       top_fuse_nodes for W in 2 .. 2048, n in 1 .. 1024, top_wide in {0, 2}.
//
// NAME=VALUE: the A/B knobs of the test build with the values the library
// would read from the environment (CDA_TOP_PAIR=0, CDA_HASH_WG_PER_CU=1, ...);
// CUS=N is the device's CU count for CDA_HASH_WG_PER_CU (default 256).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "hash_plan.h"

static const char* kernel_name(cda::PlanKernel k) {
    switch (k) {
        case cda::PlanKernel::kRs8: return "rs8";
        case cda::PlanKernel::kLeafPair: return "leaf_pair";
        case cda::PlanKernel::kLeaf: return "leaf";
        case cda::PlanKernel::kSubtree: return "subtree";
        case cda::PlanKernel::kLevel: return "level";
        case cda::PlanKernel::kTreeTop: return "tree_top";
        case cda::PlanKernel::kRfcLeaf: return "rfc_leaf";
        case cda::PlanKernel::kDataRoot: return "data_root";
    }
    return "?";
}

int main(int argc, char** argv) {
    cda::HashKnobs K;
    bool top_only = false;
    uint32_t cus = 256;
    int wg_per_cu = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--top")) {
            top_only = true;
            continue;
        }
        const char* eq = strchr(argv[i], '=');
        if (!eq) {
            fprintf(stderr, "expected NAME=VALUE, got %s\n", argv[i]);
            return 2;
        }
        const std::string name(argv[i], (size_t)(eq - argv[i]));
        const char* v = eq + 1;
        if (name == "CDA_TOP_FUSE") K.top_fuse = atoi(v);
        else if (name == "CDA_TOP_WIDE") K.top_wide = atoi(v);
        else if (name == "CDA_SUBTREE") K.subtree_min = atoi(v);
        else if (name == "CDA_SUBTREE_LANES") K.subtree_lanes = strtoull(v, nullptr, 10);
        else if (name == "CDA_HASH_SPLIT") K.hash_split = atoi(v);
        else if (name == "CDA_LEAF_PAIR_MAX") K.leaf_pair_max = strtoull(v, nullptr, 10);
        else if (name == "CDA_TOP_PAIR") K.pair = atoi(v) != 0;
        else if (name == "CDA_DR_HELPERS") K.dr_helpers = atoi(v) != 0;
        else if (name == "CDA_TOP_HELPERS") K.top_helpers = atoi(v) != 0;
        else if (name == "CDA_TOP_RFC") K.top_rfc = atoi(v) != 0;
        else if (name == "CDA_HASH_WG_PER_CU") wg_per_cu = atoi(v);
        else if (name == "CDA_RS8_ONE") K.rs8_one = atoi(v);
        else if (name == "CDA_RS8_BYTEFORM") K.rs8_byteform = atoi(v) != 0;
        else if (name == "CUS") cus = (uint32_t)atoi(v);
        else {
            fprintf(stderr, "unknown knob %s\n", name.c_str());
            return 2;
        }
    }
    K.hash_wg_cap = wg_per_cu > 0 ? (uint32_t)wg_per_cu * cus : 0u;

    if (top_only) {
        for (uint32_t W = 2; W <= 2048; W *= 2)
            for (uint32_t n = 1; n <= 1024; n++)
                for (int tw : {0, 2}) {
                    bool wide = false;
                    const uint32_t t = cda::top_fuse_nodes(W, n, K.top_fuse, tw, K.pair, &wide);
                    printf("T %u %u %d %u %d\n", W, n, tw, t, wide ? 1 : 0);
                }
        return 0;
    }
    for (uint32_t k = 1; k <= 1024; k *= 2) {
        const uint32_t n_max = k == 1024 ? 8 : k == 512 ? 32 : k == 256 ? 64 : 1024;
        for (uint32_t n = 1; n <= n_max; n++) {
            const uint32_t parts = cda::hash_parts(k, n, K.hash_split);
            for (uint32_t p = 0; p < parts; p++) {
                const cda::PartPlan P = cda::part_plan(k, n, p, K);
                printf("P %u %u %u %u %u %u %u %llu :", k, n, parts, p, P.i0, P.m, P.stop,
                       (unsigned long long)P.subtree_room);
                for (uint32_t i = 0; i < P.count; i++) {
                    const cda::PlanLaunch& L = P.launch[i];
                    printf(" %s,%u,%u,%d,%u,%u,%d,%d,%u,%u,%u,%d,%llu", kernel_name(L.kernel), L.n_in, L.sub,
                           L.wide ? 1 : 0, L.lv, L.n_dig, L.pair ? 1 : 0, L.ragged ? 1 : 0, L.pmax, L.mode, L.threads,
                           L.persistent ? 1 : 0, (unsigned long long)L.scratch);
                }
                printf("\n");
            }
        }
    }
    return 0;
}
