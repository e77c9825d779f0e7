// klt_plan.h — the launch plan of one KLT call: which kernel form runs it, with how many waves per feature, how many features
// per workgroup and how much LDS.  klt_plan() is a pure function of its input: no context, no environment, no HIP call
// (tests/test_klt_plan_cpu.py walks it without a device).
#pragma once

#include "ftk_device.h"
#include "klt_sched.h"

namespace ftk {

// Everything the decision depends on, as values.
struct KltPlanInput {
    int model, method;
    int32_t half_rows, half_cols;  // within [0, 1023] (the entry point refuses others)
    int32_t n;                     // features of the call
    int32_t max_extent;            // the largest row or column count among the pyramid levels the call walks
    int consider_luminance;
    int tree;       // the context's reduction mode is FTK_REDUCTION_TREE
    int long_tail;  // this variant's recent calls had a feature of many iterations (the tail class of the wave policy)
    // the FTK_KLT_WAVES / FTK_KLT_GROUP / FTK_LSSD_CHUNKED / FTK_KLT_SPILL overrides, already parsed, or kKltNotSet
    int waves, group, lssd_chunked, spill;
};

enum class KltForm {
    Pipelined,     // Basic KLT inverse: klt_basic_kernels.hip
    OneWaveFast,   // the `fast` method of Basic and affine KLT on one wave: klt_fast_kernels.hip
    Generic,       // klt_kernels.hip (KltParams::lssd_chunked: its chunked one-wave LSSD levels)
    GenericSpill,  // the generic kernel with its per-pixel arrays in device memory (large patches)
};

struct KltPlan {
    KltForm form;
    size_t lds_bytes;      // of a workgroup, without the sort block's minimum (klt_launch adds that)
    unsigned grid, block;  // without the sort block
};

enum KltPlanError { kKltPlanOk = 0, kKltPlanUnknownVariant, kKltPlanSpillTooLarge };

// Fills the geometry and every launch-shape field of `p` (the call's own fields — images, buffers, options — are the caller's) and
// `plan`.  On kKltPlanSpillTooLarge `spill_floats` holds the floats of device memory per feature that were asked for.
KltPlanError klt_plan(const KltPlanInput &in, KltParams *p, KltPlan *plan, size_t *spill_floats);

// Waves per feature of one call from the measured table (klt_wave_policy.inc): method_class as klt_method_class (klt_sched.h).
int klt_policy_waves(int model, int method_class, int consider_luminance, int long_tail, int pixels, int n);

// LDS bytes ONE feature needs in each form (a multiple of 16), from the geometry, waves_per_feature, tree and the carve fields of
// `p`; defined next to the kernels that carve it.  0: the form does not serve the model.
size_t klt_pipelined_feature_lds_bytes(const KltParams &p);
size_t klt_fast_feature_lds_bytes(int model, const KltParams &p);
size_t klt_generic_feature_lds_bytes(int model, const KltParams &p);
size_t klt_spill_lds_bytes(int model, const KltParams &p);
// Floats of device memory one workgroup of the large-patch form needs; 0 if the model is unknown.
size_t klt_spill_floats(int model, const KltParams &p);

// The instantiation a plan runs: its entry point and, for the tests, the compile-time choices behind it.
struct KltKernel {
    void (*entry)(const KltParams);
    const char *family;  // "pipelined", "fast", "generic"
    int half;            // compile-time half patch size (0: run-time geometry)
    bool solo;           // one wave per feature
    bool tree, lum, spill;
    bool row_chunks = false;  // the pipelined kernel's chunks are whole patch rows (klt_basic_kernels.hip pb_row_chunks)
    // the pipelined kernel: 8-byte units of the current / next reference byte window a thread prefetches at level entry (pb_octets)
    int cur_units = 0, ref_units = 0;
};
KltKernel klt_pipelined_pick(const KltParams &p);
KltKernel klt_fast_pick(int model, const KltParams &p);
KltKernel klt_pick(const KltPlan &plan, int model, int method, const KltParams &p);

// Launches the plan's kernel on `stream` (+ one workgroup for the sort of a later call's launch order when p.sort_iters is set).
hipError_t klt_launch(const KltPlan &plan, int model, int method, const KltParams &p, hipStream_t stream);

}  // namespace ftk
