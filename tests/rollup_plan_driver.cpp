/* Stand-alone driver for m3_amd/csrc/rollup_plan.h and rollup_bucket.h (no
 * HIP, no GPU). tests/test_rollup_plan.py builds it with the address and
 * undefined-behaviour sanitizers.
 *   rollup_plan_driver EPS EVERY [AGG_TYPE_ID ...]
 *     prints the plan the host layer would hand to the rollup kernels as one
 *     JSON object.
 *   rollup_plan_driver qindex EPS EVERY [AGG_TYPE_ID ...]
 *     prints exact_quantile_index for every quantile of that plan and every
 *     bucket size 1..QCAP: a JSON list of QCAP lists of nq indices.
 *   rollup_plan_driver bucket METRIC NAGGS AGG_TYPE_ID... [T V ...]
 *     accumulates the points (T V pairs) into one bucket and prints ValueOf
 *     of every aggregation as the bit pattern of the double, a JSON list. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../m3_amd/csrc/rollup_bucket.h"

template <int METRIC>
static void bucket_mode(const std::vector<int32_t>& aggs,
                        const std::vector<int64_t>& ts,
                        const std::vector<double>& vals) {
    m3::BucketState bs;
    bs.reset();
    for (size_t i = 0; i < ts.size(); i++)
        m3::bucket_add<METRIC>(bs, ts[i], vals[i]);
    printf("[");
    for (size_t i = 0; i < aggs.size(); i++) {
        double r = m3::bucket_value_of<METRIC>(bs, aggs[i]);
        uint64_t bits;
        memcpy(&bits, &r, sizeof(bits));
        printf("%s%llu", i ? ", " : "", (unsigned long long)bits);
    }
    printf("]\n");
}

static int bucket_main(int argc, char** argv) {
    if (argc < 4) return 2;
    int metric = atoi(argv[2]);
    int naggs = atoi(argv[3]);
    if (naggs < 0 || argc < 4 + naggs || (argc - 4 - naggs) % 2) return 2;
    std::vector<int32_t> aggs;
    for (int i = 0; i < naggs; i++) aggs.push_back((int32_t)atoi(argv[4 + i]));
    std::vector<int64_t> ts;
    std::vector<double> vals;
    for (int i = 4 + naggs; i < argc; i += 2) {
        ts.push_back(strtoll(argv[i], nullptr, 10));
        vals.push_back(strtod(argv[i + 1], nullptr));
    }
    switch (metric) {
    case M3GPU_METRIC_COUNTER: bucket_mode<M3GPU_METRIC_COUNTER>(aggs, ts, vals); break;
    case M3GPU_METRIC_GAUGE: bucket_mode<M3GPU_METRIC_GAUGE>(aggs, ts, vals); break;
    case M3GPU_METRIC_TIMER: bucket_mode<M3GPU_METRIC_TIMER>(aggs, ts, vals); break;
    default: return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "bucket")) return bucket_main(argc, argv);
    bool qindex = argc >= 2 && !strcmp(argv[1], "qindex");
    if (qindex) { argc--; argv++; }
    if (argc < 3 || argc - 3 > MAX_AGGS) {
        fprintf(stderr, "usage: %s [qindex] EPS EVERY [AGG_TYPE_ID ...] (at most %d)\n",
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
    if (qindex) {
        /* exactly nq quantiles on the heap, for the same reason */
        std::vector<double> qs(plan.qs, plan.qs + plan.nq);
        printf("[");
        for (int n = 1; n <= QCAP; n++) {
            printf("%s[", n > 1 ? ", " : "");
            for (int i = 0; i < plan.nq; i++)
                printf("%s%d", i ? ", " : "",
                       m3::exact_quantile_index(qs.data(), i, n));
            printf("]");
        }
        printf("]\n");
        return 0;
    }
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
