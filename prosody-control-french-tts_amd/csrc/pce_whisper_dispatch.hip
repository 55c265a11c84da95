// pce_whisper_dispatch.hip -- the Whisper / BERT / wav2vec2 entry points of include/pce.h: each forwards to the build of pce_whisper_impl.inc (and the
// .inc files it includes) the context has selected: namespace pce_bf16 (bf16 operands) or pce_f16 (fp16).  The two builds keep separate state
// (weights, buffers): switching the operand type means loading the weights again.  The forwarders are generated from the table of
// pce_whisper_entries.h; the few entry points that do not follow its rule are written out below.
#include "pce_internal.h"
#include "pce_whisper_entries.h"
#include "pce_w2v_seg_plan.h"

namespace pce_bf16 {
PCE_WHISPER_ENTRIES(PCE_DECLARE)
void pce_whisper_free(pce_ctx *c);
}
namespace pce_f16 {
PCE_WHISPER_ENTRIES(PCE_DECLARE)
void pce_whisper_free(pce_ctx *c);
int pce_w2v_check(const pce_w2v_dims *dims, int64_t n_floats, char *msg, size_t cap);
}

void pce_whisper_free(pce_ctx *c) { pce_bf16::pce_whisper_free(c); pce_f16::pce_whisper_free(c); }

#define PCE_FORWARD(name, params, args) int name params { return (c && c->whisper_ops >= 1) ? pce_f16::name args : pce_bf16::name args; }

extern "C" {

PCE_WHISPER_ENTRIES(PCE_FORWARD)

int pce_whisper_set_operands(pce_ctx *c, int32_t operand_type)
{
    if (!c) return PCE_E_INVALID;
    if (operand_type != PCE_OPERANDS_BF16 && operand_type != PCE_OPERANDS_FP16 && operand_type != PCE_OPERANDS_F16_RESID16)
        return pce_fail(c, PCE_E_INVALID, "operand type %d (0 = bf16, 1 = fp16, 2 = fp16 with the fp16 residual stream)", operand_type);
    c->whisper_ops = operand_type;
    c->resid16 = operand_type == PCE_OPERANDS_F16_RESID16;
    return PCE_OK;
}
int pce_whisper_get_operands(pce_ctx *c) { return c ? c->whisper_ops : PCE_E_INVALID; }

// (the loader's conditions are the same in both operand builds)
int pce_w2v_check(const pce_w2v_dims *dims, int64_t n_floats, char *msg, size_t cap) { return pce_f16::pce_w2v_check(dims, n_floats, msg, cap); }
// windows and kept frames of one clip: ctc_emissions.window_plan's arithmetic (true division and truncation in double)
int pce_w2v_window_plan(int64_t n_samples, int32_t window_samples, int32_t context_samples, int64_t *n_windows, int64_t *n_frames)
{
    if (n_samples < 0 || window_samples < 1 || context_samples < 0 || !n_windows || !n_frames) return PCE_E_INVALID;
    const int64_t window = window_samples, n_win = n_samples > window ? (n_samples + window - 1) / window : 1, extension = n_win * window - n_samples;
    const int64_t wf = (int64_t)((double)window / 16000.0 * 50.0);
    *n_windows = n_win;
    *n_frames = n_win * wf - (extension > 0 ? (int64_t)((double)extension / 16000.0 * 50.0) : 0);
    return PCE_OK;
}

// frames the model gives for a segment of n_samples run on max(n_samples, min_samples): the feature encoder's arithmetic (pce_w2v_seg_plan.h)
int pce_w2v_segment_frames(const pce_w2v_dims *dims, int64_t n_samples, int32_t min_samples, int64_t *n_frames)
{
    if (!dims || !n_frames || n_samples < 0 || min_samples < 0 || dims->n_conv < 1 || dims->n_conv > 8) return PCE_E_INVALID;
    for (int i = 0; i < dims->n_conv; i++)
        if (dims->conv_kernel[i] < 1 || dims->conv_stride[i] < 1) return PCE_E_INVALID;
    int64_t t[8];
    w2v_seg_layer_frames(dims->conv_kernel, dims->conv_stride, dims->n_conv, n_samples > min_samples ? n_samples : (int64_t)min_samples, t);
    *n_frames = t[dims->n_conv - 1];
    return PCE_OK;
}

} // extern "C"
