/* Stand-alone driver for m3_amd/csrc/rollup_plan.h (no HIP, no GPU).
 *   rollup_plan_driver EPS EVERY [AGG_TYPE_ID ...]
 * prints the plan the host layer would hand to the rollup kernels as one
 * JSON object. tests/test_rollup_plan.py builds it with the address and
 * undefined-behaviour sanitizers. */
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../m3_amd/csrc/rollup_plan.h"

int main(int argc, char** argv) {
    if (argc < 3 || argc - 3 > MAX_AGGS) {
        fprintf(stderr, "usage: %s EPS EVERY [AGG_TYPE_ID ...] (at most %d)\n",
                argv[0], MAX_AGGS);
        return 2;
    }
    double eps = atof(argv[1]);
    int every = atoi(argv[2]);
    /* exactly naggs elements on the heap: a read past them is an
     * AddressSanitizer report */
    std::vector<int32_t> aggs;
    for (int i = 3; i < argc; i++) aggs.push_back((int32_t)atoi(argv[i]));
    int naggs = (int)aggs.size();
    m3::RollupPlan plan;
    m3::rollup_plan_build(aggs.data(), naggs, eps, every, &plan);
    printf("{\"nq\": %d, \"qs\": [", plan.nq);
    for (int i = 0; i < plan.nq; i++)
        printf("%s%.17g", i ? ", " : "", plan.qs[i]);
    printf("], \"qidx\": [");
    for (int i = 0; i < naggs; i++)
        printf("%s%d", i ? ", " : "", (int)plan.qidx[i]);
    printf("], \"exact_cap\": %d, \"extreme_cap\": %d}\n", plan.exact_cap,
           plan.extreme_cap);
    return 0;
}
