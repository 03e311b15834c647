// zeggs_set_option: every process-wide switch of the library, one row each.  The switches themselves live beside the code that
// reads them; this file is the one place that declares them all.
#include "../../include/zeggs_hip.h"
#include "common.h"
#include "decoder_ws.h"

extern int g_attn_bwd_one_launch, g_fused_attention;                                          // attention.hip
extern int g_decoder_fast, g_bwd_chunks, g_tp_prologue, g_wgrad_order;                        // decoder.hip
extern int g_stage_variant, g_timing, g_chain, g_sweep_graphs, g_launch_window;               // decoder_fast.hip
extern int g_tp_tiles4, g_tp_dual;                                                            // train_persistent.hip, train_dual.hip
extern int g_gemm_wg_target, g_gemm_streamk_wgs, g_gemm_mid_split, g_gemm_skinny, g_gemm_streamk, g_gemm_split_bf16;   // gemm*.hip
extern int g_text_emit, g_text_passes;                                                          // text.hip
extern int g_mel_mfma, g_mel_fft, g_mel_exact_log, g_loss_lds, g_ln_bwd4;                     // mel.hip, loss.hip, kernels.hip
void zeggs_gemm_set_dma(int on), zeggs_gemm_set_direct(int mode, int wgs), zeggs_gemm_set_direct_depth(int d);           // gemm.hip
void zeggs_gemm_set_direct_shield(int on), zeggs_gemm_set_direct_reserve(int n), zeggs_gemm_set_asum(int on);

namespace {
enum Kind { AS_GIVEN, NONZERO, MIN0, MIN1, CALL };      // *target = v, v != 0, max(0, v), max(1, v); CALL: set(v), not a plain store
struct Option { const char* name; int* target; Kind kind; int (*set)(int); };
int set_chain(int v) {
#ifndef ZEGGS_CHAIN
  if (v) { zeggs_set_error("option chain: the chained (run-ahead) stage launches lost to the persistent decode kernel and are "
                           "compiled in measurement builds only (-DZEGGS_CHAIN)"); return -1; }
#endif
  g_chain = v;
  return 0;
}
const Option k_options[] = {
  {"attn_bwd_one_launch", &g_attn_bwd_one_launch, NONZERO},
  {"decoder_fast", &g_decoder_fast, AS_GIVEN},
  {"stage_variant", &g_stage_variant, AS_GIVEN},
  {"gemm_wg_target", &g_gemm_wg_target, AS_GIVEN},
  {"timing", &g_timing, AS_GIVEN},
  {"chain", nullptr, CALL, set_chain},
  {"sweep_graphs", &g_sweep_graphs, NONZERO},
  {"launch_window", &g_launch_window, MIN0},
  {"train_persistent", nullptr, CALL, [](int v) { g_sweep_kernels[SWEEP_ROLLOUT].set_enabled(v); return 0; }},
  {"bwd_persistent", nullptr, CALL, [](int v) { g_sweep_kernels[SWEEP_BPTT].set_enabled(v); return 0; }},
  {"persistent", nullptr, CALL, [](int v) { g_sweep_kernels[SWEEP_DECODE].set_enabled(v); return 0; }},
  {"mel_mfma", &g_mel_mfma, NONZERO},
  {"mel_fft", &g_mel_fft, NONZERO},
  {"gemm_streamk_wgs", &g_gemm_streamk_wgs, AS_GIVEN},
  {"gemm_mid_split", &g_gemm_mid_split, NONZERO},
  {"gemm_dma", nullptr, CALL, [](int v) { zeggs_gemm_set_dma(v != 0); return 0; }},
  {"gemm_direct", nullptr, CALL, [](int v) { zeggs_gemm_set_direct(v, -1); return 0; }},
  {"gemm_direct_wgs", nullptr, CALL, [](int v) { zeggs_gemm_set_direct(-1, v); return 0; }},
  {"gemm_direct_depth", nullptr, CALL, [](int v) { zeggs_gemm_set_direct_depth(v); return 0; }},
  {"gemm_direct_shield", nullptr, CALL, [](int v) { zeggs_gemm_set_direct_shield(v); return 0; }},
  {"gemm_direct_reserve", nullptr, CALL, [](int v) { zeggs_gemm_set_direct_reserve(v); return 0; }},
  {"gemm_asum", nullptr, CALL, [](int v) { zeggs_gemm_set_asum(v); return 0; }},
  {"gemm_skinny", &g_gemm_skinny, NONZERO},
  {"gemm_streamk", &g_gemm_streamk, NONZERO},
  {"fused_attention", &g_fused_attention, NONZERO},
  {"bwd_chunks", &g_bwd_chunks, MIN1},
  {"tp_tiles4", &g_tp_tiles4, NONZERO},
  {"tp_dual", &g_tp_dual, NONZERO},
  {"tp_prologue", &g_tp_prologue, NONZERO},
  {"loss_lds", &g_loss_lds, NONZERO},
  {"wgrad_order", &g_wgrad_order, AS_GIVEN},
  {"gemm_split_bf16", nullptr, CALL, [](int v) { g_gemm_split_bf16 = (v == 3 || v == 6 || v == 9) ? v : 0; return 0; }},
  {"poll_stagger", &g_poll_stagger, MIN0},
  {"poll_sleep", &g_poll_sleep, MIN0},
  // bound of every device-side wait of the persistent kernels (polls); 0 makes the first unsatisfied wait give up: the
  // tests use it to drive the give-up path (tests/test_gpu_giveup.py)
  {"persistent_spin", &g_persistent_spin, MIN0},
  {"ln_bwd4", &g_ln_bwd4, AS_GIVEN},
  {"mel_exact_log", &g_mel_exact_log, AS_GIVEN},
  // device BVH text: text_emit 1 = the LDS-assembly emit variant (0: per-byte stores); text_passes: bit mask measure / scan / emit (tools/bvh_text_bench.py only)
  {"text_emit", &g_text_emit, AS_GIVEN},
  {"text_passes", &g_text_passes, AS_GIVEN},
};
}  // namespace

extern "C" int zeggs_set_option(const char* name, int value) {
  for (const Option& o : k_options) {
    if (strcmp(name, o.name) != 0) continue;
    if (o.kind == CALL) return o.set(value);
    const int lo = o.kind == MIN1 ? 1 : 0;
    *o.target = o.kind == AS_GIVEN ? value : o.kind == NONZERO ? value != 0 : value < lo ? lo : value;
    return 0;
  }
  zeggs_set_error("unknown option %s", name);
  return -1;
}
