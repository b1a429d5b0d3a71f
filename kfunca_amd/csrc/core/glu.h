// namespace gpu: gated activations (kf_glu_fwd, kf_glu_bwd) with autograd. No reference counterpart: the non-linearity of a Llama /
// Mistral / Gemma-family MLP, between the gate | up projection and the down projection.
#pragma once

#include <cstdint>

#include "tensor.h"

namespace gpu {

// act: KF_ACT_SILU, KF_ACT_GELU_TANH or KF_ACT_GELU_ERF.
// glu(act, gate, up): h = act(gate) * up for two tensors of one shape [..., F]. up undefined: gate is the packed projection [..., 2F]
// (columns gate | up) and the result is [..., F]. Operands with a unit stride along the last dim and one uniform row stride over the
// flattened leading dims (the halves Tensor::split returns from a packed projection, a column slice) are read in place through their
// leading dimension; anything else is made dense first. The result is a new dense tensor. The backward is ONE kf_glu_bwd launch that
// recomputes the activation from the kept inputs: the packed form returns one [..., 2F] gradient, the two-tensor form dgate and dup.
Tensor glu(int act, const Tensor &gate, const Tensor &up);
// the ungated act(x), any shape [..., F]
Tensor activation(int act, const Tensor &x);

} // namespace gpu
