"""CPU checks of the layer output error behind an inserted transformation (compare_layer_outputs with
follow_input_transforms): that the inserted ops are recognised and their constants handed to the kernels as stored, so
that the reported error is the one an evaluation straight from the tokens gives (m against 1/m shows here); the
unchanged default, every refusal, the argument errors of mi355q_weight_delta_transformed_f32, and that
csrc/hadamard.hip compiles for gfx950 without scratch. The kernels are float64 NumPy stand-ins, which apply the constant
themselves: how the real kernel applies it is tests/test_gpu_layer_error_transforms.py's business."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import layer_error_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-edge-quantizer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

D, DKV, DFF = 128, 32, 256
TODAY = ["d", "error", "input", "output_mse", "output_snr", "per_channel_error", "rows", "signal", "weight"]


def _kernels():
  from mi355q import model_validator as mv
  from mi355q.transformations import graph_edits

  class Float64Kernels(mv.LayerErrorKernels):
    """The device side in float64 throughout: nothing is rounded to float32 but what the model stores."""
    transformed = []

    def weight(self, values):
      return np.asarray(values, np.float64)

    def _dequant(self, plan):
      return LC.dequantize(np.asarray(plan.data), plan.scale, plan.zero_point, plan.channels, plan.inner,
                           plan.diff_bits).astype(np.float64)

    def delta(self, reference, plan):
      if plan.kind == "f32":
        return reference - np.asarray(plan.data, np.float64)
      return reference - self._dequant(plan)

    def delta_transformed(self, reference, plan, d, multiplier, hadamard_size):
      Float64Kernels.transformed.append((plan.name, multiplier is not None, hadamard_size))
      dq = self._dequant(plan).reshape(-1, d)
      if multiplier is not None:
        assert hadamard_size == 0 and multiplier.dtype == np.float32 and multiplier.shape == (d,)
        dq = dq * multiplier.astype(np.float64)
      else:
        h = hadamard_size
        matrix = graph_edits._sylvester_hadamard_f32(h).astype(np.float64)      # pylint: disable=protected-access
        dq = (dq.reshape(-1, h) @ matrix).reshape(-1, d)
      return reference - dq.ravel()

    def hessian(self, stat):
      return np.asarray(stat, np.float64), 1.0

    def quadform(self, a, rows, d, product, alpha):
      return LC.exact_rows(np.asarray(a).reshape(rows, d), LC.symmetric(product), alpha)
  Float64Kernels.transformed = []
  return Float64Kernels


def _tensor_id(model, name):
  return next(i for i, t in enumerate(model.subgraphs[0].tensors) if t.name.decode() == name)


def _tensor(model, name):
  return model.subgraphs[0].tensors[_tensor_id(model, name)]


def _weight(model, name):
  t = _tensor(model, name)
  return np.asarray(model.buffers[t.buffer].data).view(np.float32).reshape(t.shape).copy()


def _store_int8(model, name, values):
  """Rewrites constant `name` as channelwise int8 of `values`; returns the float32 dequantized values."""
  from mi355q import qtyping as q
  t = _tensor(model, name)
  values = np.asarray(values, np.float64)
  scale = (np.abs(values).max(axis=1) / 100.0).astype(np.float32)
  ints = np.clip(np.rint(values / scale[:, None]), -128, 127).astype(np.int8)
  t.type = int(q.TensorType.INT8)
  t.quantization = q.QuantizationParametersT(scale=scale, zeroPoint=np.zeros(len(scale), np.int64), quantizedDimension=0)
  model.buffers[t.buffer].data = ints.reshape(-1).view(np.uint8)
  return LC.dequantize(ints, scale, None, values.shape[0], values.shape[1], 32).reshape(values.shape)


def _insert(model, how, x_name, ops, **params):
  """Inserts a transformation after activation `x_name` for the FULLY_CONNECTED ops named `ops`, through graph_edits."""
  from mi355q import qtyping as q
  from mi355q.transformations import graph_edits, transformation_utils
  sg = model.subgraphs[0]
  tid = _tensor_id(model, x_name)
  outs = {_tensor_id(model, f"l0/{n}/y") for n in ops}
  consumers = [i for i, op in enumerate(sg.operators) if op.inputs[0] == tid and op.outputs[0] in outs]
  assert len(consumers) == len(ops)
  hadamard = None
  if "h" in params:
    signs = params.get("signs", np.ones(params["h"], np.int8))
    hadamard = q.UniformQuantParams.HadamardRotationParams(signs, params["h"])
  custom = {"multiplier": params["multiplier"]} if "multiplier" in params else None
  qp = q.UniformQuantParams(num_bits=8, quantized_dimension=0, scale=np.ones(1, np.float32), zero_point=np.zeros(1, np.int64),
                            hadamard=hadamard, custom_algorithm_param=custom)
  ti = transformation_utils.TransformationInput(tid, model, sg, -1, consumers, qp)
  fn = {"multiply": graph_edits.insert_multiply, "custom": graph_edits.insert_hadamard_rotation,
        "decomposed": graph_edits.insert_decomposed_hadamard_rotation}[how]
  return fn(ti)


def _rotate(values, h):
  from mi355q.transformations import graph_edits
  matrix = graph_edits._sylvester_hadamard_f32(h).astype(np.float64)      # pylint: disable=protected-access
  return (np.asarray(values, np.float64).reshape(-1, h) @ matrix).reshape(np.shape(values))


H_CUSTOM, H_DECOMPOSED = 64, 32      # 1/sqrt(64) is a float32, 1/sqrt(32) is not


def _models():
  """Float model and a target with o behind a MUL, down behind the custom op, gate / up behind the decomposed chain,
  q / k / v untransformed; the multiplier and the float32 dequantized weights of the target."""
  import c5_model as C
  ref, tgt = C.build_model(1, d=D, dkv=DKV, dff=DFF), C.build_model(1, d=D, dkv=DKV, dff=DFF)
  rng = np.random.default_rng(31)
  m = np.exp(rng.uniform(-1.0, 1.0, D)).astype(np.float32)      # 0.37 .. 2.7: m and 1/m are far apart
  deq = {}
  for name in ("q", "k", "v"):
    deq[name] = _store_int8(tgt, f"l0/{name}/w", _weight(ref, f"l0/{name}/w"))
  deq["o"] = _store_int8(tgt, "l0/o/w", _weight(ref, "l0/o/w").astype(np.float64) / m.astype(np.float64))
  deq["down"] = _store_int8(tgt, "l0/down/w", _rotate(_weight(ref, "l0/down/w"), H_CUSTOM))
  for name in ("gate", "up"):
    deq[name] = _store_int8(tgt, f"l0/{name}/w", _rotate(_weight(ref, f"l0/{name}/w"), H_DECOMPOSED))
  _insert(tgt, "multiply", "l0/o_in", ["o"], multiplier=m)
  _insert(tgt, "custom", "l0/down_in", ["down"], h=H_CUSTOM)
  _insert(tgt, "decomposed", "l0/mlp_in", ["gate", "up"], h=H_DECOMPOSED)
  return C, ref, tgt, m, deq


def _tokens_and_hessians(C):
  tokens, qsvs = {}, {}
  for _, _, cols, src in C.projections(D, DKV, DFF):
    if src not in tokens:
      x = np.concatenate([s[0] for s in LC.tokens(cols, 200 + len(tokens))], axis=0).astype(np.float64)
      tokens[src] = x
      qsvs[f"l0/{src}"] = {"hessian": (2.0 / x.shape[0]) * x.T @ x, "num_samples": np.array(x.shape[0])}
  return tokens, qsvs


EXPECTED = {"q": ("none", 0), "k": ("none", 0), "v": ("none", 0), "o": ("multiply", 0), "gate": ("hadamard", H_DECOMPOSED),
            "up": ("hadamard", H_DECOMPOSED), "down": ("hadamard", H_CUSTOM)}


def test_error_is_the_output_error_of_the_graph_as_it_applies_the_transformation():
  from mi355q import model_validator as mv
  from mi355q.transformations import graph_edits
  from mi355q.utils import tfl_flatbuffer_utils
  C, ref, tgt, m, deq = _models()
  tokens, qsvs = _tokens_and_hessians(C)
  kernels = _kernels()
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=kernels(), follow_input_transforms=True)
  assert not got.skipped and len(got) == 7
  sg = tgt.subgraphs[0]
  for name, rows, d, src in C.projections(D, DKV, DFF):
    r = got[f"l0/{name}/y"]
    assert sorted(r) == sorted(TODAY + ["input_transform", "hadamard_size"])
    assert (r["input_transform"], r["hadamard_size"]) == EXPECTED[name]
    assert (r["weight"], r["input"], r["rows"], r["d"]) == (f"l0/{name}/w", f"l0/{src}", rows, d)
    x = tokens[src]
    n = x.shape[0]
    # T(X) from the graph's own constants, in float64
    if name == "o":
      stored = next(t for t in sg.tensors if t.name == b"l0/o_in_multiplier")
      tx = x * np.asarray(tfl_flatbuffer_utils.get_tensor_data(stored, tgt.buffers), np.float64).reshape(1, d)
    elif EXPECTED[name][0] == "hadamard":
      h = EXPECTED[name][1]
      if name == "down":
        matrix = graph_edits._sylvester_hadamard_f32(h)      # pylint: disable=protected-access
      else:
        stored = next(t for t in sg.tensors if t.name == b"l0/mlp_in_hadamard_matrix")
        matrix = np.asarray(tfl_flatbuffer_utils.get_tensor_data(stored, tgt.buffers)).reshape(h, h)
      tx = (x.reshape(-1, h) @ matrix.astype(np.float64)).reshape(n, d)
    else:
      tx = x
    w = _weight(ref, f"l0/{name}/w").astype(np.float64)
    want = np.sum((x @ w.T - tx @ deq[name].astype(np.float64).T) ** 2) / n
    print(f"l0/{name}: {r['input_transform']} h={r['hadamard_size']} error {r['error']:.6e}, from the tokens {want:.6e},"
          f" relative {abs(r['error'] - want) / want:.2e}")
    np.testing.assert_allclose(r["error"], want, rtol=1e-9)
    assert r["error"] == float(np.sum(r["per_channel_error"])) and r["error"] > 0
    # the quantization is int8: a transformation applied the wrong way round is orders of magnitude away
    assert r["error"] < 1e-3 * r["signal"]
  assert sorted(kernels.transformed) == [("l0/down/w", False, H_CUSTOM), ("l0/gate/w", False, H_DECOMPOSED),
                                         ("l0/o/w", True, 0), ("l0/up/w", False, H_DECOMPOSED)]


def test_default_call_is_unchanged():
  from mi355q import model_validator as mv
  C, ref, tgt, _, _ = _models()
  _, qsvs = _tokens_and_hessians(C)
  for kw in ({}, {"follow_input_transforms": False}):
    kernels = _kernels()
    got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=kernels(), **kw)
    assert got.skipped == {f"l0/{n}/y": mv.SKIP_INPUT for n in ("o", "gate", "up", "down")}
    assert sorted(got) == ["l0/k/y", "l0/q/y", "l0/v/y"] and not kernels.transformed
    for r in got.results.values():
      assert sorted(r) == TODAY


def test_stand_ins_that_know_only_delta_keep_working():
  """delta_transformed is called only when a transformation was found."""
  from mi355q import model_validator as mv
  import c5_model as C
  ref, tgt = C.build_model(1, d=D, dkv=DKV, dff=DFF), C.build_model(1, d=D, dkv=DKV, dff=DFF)
  _store_int8(tgt, "l0/q/w", _weight(ref, "l0/q/w"))
  base = _kernels()

  class OnlyDelta(base):
    def delta_transformed(self, *args):
      raise AssertionError("no transformation in this model")
  _, qsvs = _tokens_and_hessians(C)
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=OnlyDelta(), follow_input_transforms=True)
  assert not got.skipped and len(got) == 7
  assert all(r["input_transform"] == "none" and r["hadamard_size"] == 0 for r in got.results.values())
  assert got["l0/q/y"]["error"] > 0 and got["l0/k/y"]["error"] == 0.0


def test_hadamard_size_one_is_no_rotation():
  from mi355q import model_validator as mv
  import c5_model as C
  ref, tgt = C.build_model(1, d=D, dkv=DKV, dff=DFF), C.build_model(1, d=D, dkv=DKV, dff=DFF)
  _store_int8(tgt, "l0/o/w", _weight(ref, "l0/o/w"))
  _insert(tgt, "custom", "l0/o_in", ["o"], h=1)
  _, qsvs = _tokens_and_hessians(C)
  kernels = _kernels()
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=kernels(), follow_input_transforms=True)
  plain = mv.compare_layer_outputs(ref, C.build_model(1, d=D, dkv=DKV, dff=DFF), qsvs, kernels=kernels())
  assert not got.skipped and not kernels.transformed
  assert (got["l0/o/y"]["input_transform"], got["l0/o/y"]["hadamard_size"]) == ("none", 0)
  assert got["l0/o/y"]["error"] > 0 and got["l0/o/y"]["signal"] == plain["l0/o/y"]["signal"]


def _refuse_short_multiplier(tgt):
  _insert(tgt, "multiply", "l0/o_in", ["o"], multiplier=np.full(D // 2, 1.5, np.float32))


def _refuse_flipped_matrix(tgt):
  _insert(tgt, "decomposed", "l0/o_in", ["o"], h=32)
  t = _tensor(tgt, "l0/o_in_hadamard_matrix")
  matrix = np.array(np.asarray(tgt.buffers[t.buffer].data).view(np.float32))
  matrix[5 * 32 + 7] = -matrix[5 * 32 + 7]
  tgt.buffers[t.buffer].data = matrix.view(np.uint8)


def _refuse_minus_one(tgt):
  signs = np.ones(32, np.int8)
  signs[3] = -1
  _insert(tgt, "custom", "l0/o_in", ["o"], h=32, signs=signs)


def _refuse_other_producer(tgt):
  from mi355q import qtyping as q
  from mi355q.transformations import transformation_utils
  info = _insert(tgt, "multiply", "l0/o_in", ["o"], multiplier=np.full(D, 1.5, np.float32))
  op = tgt.subgraphs[0].operators[info.op_id]
  op.opcodeIndex = transformation_utils.add_op_code(q.BuiltinOperator.ADD, tgt.operatorCodes, "ADD")


def _refuse_size_that_does_not_divide(tgt):
  _insert(tgt, "custom", "l0/o_in", ["o"], h=2 * D)


def _refuse_multiply_with_a_fused_activation(tgt):
  info = _insert(tgt, "multiply", "l0/o_in", ["o"], multiplier=np.full(D, 1.5, np.float32))
  tgt.subgraphs[0].operators[info.op_id].builtinOptions.fusedActivationFunction = 1      # RELU


def _refuse_vector_shorter_than_the_size(tgt):
  _insert(tgt, "custom", "l0/o_in", ["o"], h=32, signs=np.ones(16, np.int8))


def _refuse_rotation_with_a_bias(tgt):
  from mi355q.transformations import transformation_utils
  from mi355q import qtyping as q
  info = _insert(tgt, "decomposed", "l0/o_in", ["o"], h=32)
  sg = tgt.subgraphs[0]
  bias = transformation_utils.add_new_constant_tensor(b"bias", np.zeros(32, np.float32), q.TensorType.FLOAT32, sg, tgt)
  fc = sg.operators[info.op_id + 1]
  fc.inputs = list(fc.inputs) + [bias]


def _refuse_reshape_to_another_width(tgt):
  info = _insert(tgt, "decomposed", "l0/o_in", ["o"], h=32)
  sg = tgt.subgraphs[0]
  sg.tensors[sg.operators[info.op_id].outputs[0]].shape = [2, 64]


def _refuse_chain_of_two(tgt):
  _insert(tgt, "multiply", "l0/o_in", ["o"], multiplier=np.full(D, 1.5, np.float32))
  _insert(tgt, "multiply", "l0/o_in_scaled", ["o"], multiplier=np.full(D, 0.5, np.float32))


@pytest.mark.parametrize("edit", [_refuse_short_multiplier, _refuse_flipped_matrix, _refuse_minus_one,
                                  _refuse_other_producer, _refuse_size_that_does_not_divide, _refuse_chain_of_two,
                                  _refuse_multiply_with_a_fused_activation, _refuse_vector_shorter_than_the_size,
                                  _refuse_rotation_with_a_bias, _refuse_reshape_to_another_width],
                         ids=lambda f: f.__name__[len("_refuse_"):])
def test_refusals_with_the_flag_on(edit):
  from mi355q import model_validator as mv
  import c5_model as C
  ref, tgt = C.build_model(1, d=D, dkv=DKV, dff=DFF), C.build_model(1, d=D, dkv=DKV, dff=DFF)
  _store_int8(tgt, "l0/o/w", _weight(ref, "l0/o/w"))
  edit(tgt)
  _, qsvs = _tokens_and_hessians(C)
  kernels = _kernels()
  got = mv.compare_layer_outputs(ref, tgt, qsvs, kernels=kernels(), follow_input_transforms=True)
  assert got.skipped == {"l0/o/y": mv.SKIP_INPUT} and len(got) == 6 and not kernels.transformed


def test_quantizer_passes_the_flag_through(monkeypatch):
  from mi355q import model_validator as mv
  from mi355q import quantizer
  ref = open(os.path.join(ROOT, "tests", "golden", "models", "single_fc_bias.tflite"), "rb").read()
  qz = quantizer.Quantizer(ref)
  qz._result = quantizer.QuantizationResult([{}], bytearray(ref))      # pylint: disable=protected-access
  monkeypatch.setattr(mv, "LayerErrorKernels", _kernels())
  x = np.random.default_rng(2).standard_normal((12, 8))
  qsvs = {"serving_default_input_2:0": {"hessian": 0.5 * x.T @ x, "num_samples": np.array(4)}}
  off = qz.validate_layer_outputs(calibration_result=qsvs)
  on = qz.validate_layer_outputs(calibration_result=qsvs, follow_input_transforms=True)
  (r_off,), (r_on,) = off.results.values(), on.results.values()
  assert sorted(r_off) == TODAY and (r_on["input_transform"], r_on["hadamard_size"]) == ("none", 0)
  assert on.as_dict()["layers"]["StatefulPartitionedCall:0"]["input_transform"] == "none"


# ---------------------------------------------------------------- the C entry's arguments
def test_argument_errors_of_the_transformed_delta_without_a_device():
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  g.build()
  from mi355q import _ffi
  lib = _ffi.lib()
  buf = ctypes.create_string_buffer(256)
  p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
  err = lib.mi355q_last_error
  I8, F32 = 3, 0

  def call(reference=p, target=p, n=64, kind=I8, diff_bits=32, channels=4, inner=16, scale=p, zero_point=None, d=16,
           multiplier=None, h=0, out=p):
    return lib.mi355q_weight_delta_transformed_f32(reference, target, n, kind, diff_bits, channels, inner, scale,
                                                   zero_point, d, multiplier, h, out, None)
  assert call(n=-1) == -1 and b"negative element count" in err()
  assert call(d=0) == -1 and b"d must be >= 1" in err()
  assert call(d=24) == -1 and b"not a multiple of the row length" in err()
  for h in (3, 12, -2):
    assert call(h=h) == -1 and b"power of 2" in err()
  assert call(h=32) == -1 and b"does not divide the row length" in err()
  assert call(n=1 << 16, d=1 << 15, h=1 << 15) == -1 and b"16384" in err()
  assert call(multiplier=p, h=4) == -3 and b"a multiplier and a rotation at once" in err()
  for h in (0, 1):      # no rotation: a multiplier alone is fine as far as the shapes go; the pointers are looked at next
    assert call(multiplier=p, h=h, reference=None) == -1 and b"null pointer" in err()
  for null in ("reference", "target", "out"):
    assert call(**{null: None}) == -1 and b"null pointer" in err()
  assert call(kind=8) == -1 and b"unknown target kind 8" in err()
  assert call(kind=-1) == -1 and b"unknown target kind" in err()
  assert call(scale=None) == -1 and b"integer target without scales" in err()
  assert call(channels=0) == -1 and b"channels and inner must be >= 1" in err()
  assert call(inner=0) == -1 and b"channels and inner must be >= 1" in err()
  assert call(diff_bits=12) == -1 and b"diff_bits must be 8, 16 or 32" in err()
  # an empty tensor enqueues nothing, whatever the pointers
  assert call(n=0, reference=None, target=None, out=None, scale=None) == 0 and err() == b""
  assert call(n=0, reference=None, target=None, out=None, kind=F32, h=16) == 0 and err() == b""


# ---------------------------------------------------------------- the kernels' build
@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_hadamard_kernels_use_no_scratch(tmp_path):
  sys.path.insert(0, ROOT)
  import __graft_entry__ as g
  assert "hadamard.hip" in g.SOURCES
  out = str(tmp_path / "hadamard.s")
  cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", *g.COMPILE_FLAGS, "--cuda-device-only", "-S",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(CSRC, "hadamard.hip"), "-o", out]
  subprocess.run(cmd, check=True, capture_output=True)
  with open(out) as f:
    asm = f.read()
  kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
  sizes = re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", asm)
  assert kernels and len(kernels) == len(sizes) and all(int(s) == 0 for s in sizes), (kernels, sizes)
  assert not re.search(r"\.amdhsa_uses_dynamic_stack\s+1", asm)
