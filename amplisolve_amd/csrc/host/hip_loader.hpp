// amplisolve_amd/csrc/host/hip_loader.hpp -- run-time binding of libamplisolve_hip.so (include/amplisolve_hip.h).
// The host library must load on a machine without ROCm devices (parsers, writers and their tests run there);
// every compute entry point goes through this table and fails loudly when the library is absent.
#pragma once
#include <string>

#include "../../../include/amplisolve_hip.h"

// The entry points the host library calls, in the order they are bound.  X(name): field `name`, bound to ampli_<name>;
// XAS(field, name): the same under another field name.  A field takes its type from the header's prototype, so a call whose
// arguments no longer match the header does not compile.  Every entry is required: one missing symbol fails the whole load.
#define AMPLI_HIP_API(X, XAS)                                                                                                     \
    X(abi_version) XAS(strerror_, strerror) X(device_count) X(ctx_create) X(ctx_destroy) X(last_error) X(sync) X(pinned_alloc)    \
    X(pinned_free) X(host_register) X(host_unregister) X(dev_alloc) X(dev_free) X(copy_h2d) X(copy_d2h) X(memset_d) X(acc_bytes)  \
    X(acc_bind) X(error_reduce) X(error_finalize) X(error_estimate) X(slice_len) X(slice_bytes) X(error_reduce_sliced)            \
    X(error_finalize_slice) X(error_table_unslice) X(poisson_call) X(set_tuning) X(ctx_flags) X(set_queue_items)                  \
    X(error_reduce_records) X(poisson_call_records) X(acc_to_slices) X(error_reduce_records_sliced) X(last_reduce_kernel)         \
    X(error_sums_inorder) X(loo_call_records) X(mem_info) X(limit_records) X(power_records) X(power_stats) X(dispersion_records)  \
    X(dispersion_finalize) X(genotype_planes_records) X(concordance_pairs) X(contamination_records) X(amplicon_depth_records)     \
    X(amplicon_reference) X(amplicon_ratio) X(spectrum_records) X(exceedance_records) X(overdispersion_records)                   \
    X(overdispersion_finalize) X(nb_score_records) X(pair_score_records) X(fdr_workspace_bytes) X(fdr_adjust) X(dilute_records)   \
    X(monitor_sums_records) X(monitor_control_records) X(monitor_score)                                                           \
    X(hetsite_reference_records) X(allelic_site_records) X(allelic_region_sums) X(fraction_records)                               \
    X(event_create) X(event_destroy) X(event_record) X(event_sync) X(pileup_count) X(pileup_indel_count) X(comm_create)           \
    X(comm_destroy) X(pileup_amplicon_count) X(amplicon_layers) X(pileup_evidence) X(evidence_score)                              \
    X(pileup_phase) X(phase_score)                                                                                                \
    X(comm_reduce_scatter_f64) X(comm_all_to_all_f32) X(comm_all_gather_bytes) X(comm_all_reduce_max_i32)                         \
    X(comm_exclusive_sum_i64) X(comm_barrier)

namespace ampli {

struct HipApi {
#define AMPLI_HIP_FIELD_AS(field, name) decltype(&::ampli_##name) field;
#define AMPLI_HIP_FIELD(name) AMPLI_HIP_FIELD_AS(name, name)
    AMPLI_HIP_API(AMPLI_HIP_FIELD, AMPLI_HIP_FIELD_AS)
#undef AMPLI_HIP_FIELD
#undef AMPLI_HIP_FIELD_AS
};

const HipApi *hip_api(std::string *why);

} // namespace ampli
