"""INTEGRATION.md section 3 says the reference's OWN objects can be handed to this package's functions (they only use
attribute access on `op_info` / `tensor_quant_config`, and the enums compare by value). This makes that a tested
statement for the host-only entries -- the ones that run without a GPU: `tensor_zp_scale_from_min_max` (a2), the
activation branch of `get_tensor_quant_params` (a4, tensor_content None), the QSV merges (a9) and the recipe manager.

The foreign objects are built from what tests/golden/ref_foreign_objects.json recorded of the reference's qtyping: its
enums (str enums of their own class, members and values as the reference has them) and its frozen dataclasses (the
reference's field names, order and defaults). None of them is this package's type. What the reference returned for the
same calls on its own objects is recorded beside them (.json / .npz, written by tests/golden/gen/make_foreign_objects_golden.py
from the real reference; the cases' inputs are made by the functions of this module, there and here).
Ref: algorithm_manager_api.py:191-227, qtyping.py:205-313, 384-445, 567-581, 701-710."""
import dataclasses
import enum
import json
import os
import types

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ZP_SCALE_CASES = [(gran, bits, symmetric) for gran in ("TENSORWISE", "CHANNELWISE", "BLOCKWISE_32", "BLOCKWISE_128")
                  for bits, symmetric in ((8, True), (8, False), (4, True), (4, False), (16, True))]
ACTIVATION_CASES = [(8, False), (8, True), (16, True)]
QSV_MERGES = ("moving_average_update", "min_max_update")
RECIPE_LOOKUPS = [(scope, op) for scope in ("model/mlp/fc;", "model/attn/q;", "other;")
                  for op in ("FULLY_CONNECTED", "CONV_2D")]


# ---- the cases' inputs (shared with the fixture generator)
def zp_scale_inputs(gran, bits):
  rng = np.random.default_rng(bits * 7 + len(gran))
  shape = (6, 5) if gran.startswith("BLOCKWISE") else (6, 1) if gran == "CHANNELWISE" else (1, 1)
  lo = -np.abs(rng.standard_normal(shape)).astype(np.float32) * 3
  hi = np.abs(rng.standard_normal(shape)).astype(np.float32) * 3
  lo[0, 0], hi[0, 0] = 0.0, 0.0                         # the 1e-9 floor
  return lo, hi, (None, np.full(shape, 1.5, np.float32))


def zp_scale_key(gran, bits, symmetric, clip):
  return f"zp_scale/{gran}/{bits}/{int(symmetric)}/{'noclip' if clip is None else 'clip'}"


def activation_qsv():
  return {"min": np.array([[-1.25]], np.float32), "max": np.array([[3.5]], np.float32)}


def activation_key(bits, symmetric):
  return f"activation/{bits}/{int(symmetric)}"


def qsv_pairs():
  rng = np.random.default_rng(3)
  for i in range(50):
    a = {"min": rng.standard_normal((1, 1)).astype(np.float32), "max": rng.standard_normal((1, 1)).astype(np.float32)}
    b = {"min": rng.standard_normal((1, 1)).astype(np.float32), "max": rng.standard_normal((1, 1)).astype(np.float32)}
    yield i, a, b


def fill_recipe(rm, Q):
  """Scopes added with the given qtyping's op names / configs (the reference's, or the foreign stand-ins of it)."""
  w8 = Q.OpQuantizationConfig(weight_tensor_config=Q.TensorQuantizationConfig(num_bits=8, symmetric=True,
                                                                              granularity=Q.QuantGranularity.CHANNELWISE),
                              compute_precision=Q.ComputePrecision.INTEGER)
  w4 = Q.OpQuantizationConfig(weight_tensor_config=Q.TensorQuantizationConfig(num_bits=4, symmetric=True,
                                                                              granularity=Q.QuantGranularity.BLOCKWISE_32),
                              compute_precision=Q.ComputePrecision.INTEGER)
  rm.add_quantization_config(".*", Q.TFLOperationName.FULLY_CONNECTED, op_config=w8)
  rm.add_quantization_config(".*/attn/.*", Q.TFLOperationName.FULLY_CONNECTED, op_config=w4)


# ---- the foreign objects
class _FrozenMap(dict):
  """A hashable mapping, as the reference's configs hold their algorithm_params in."""

  def __hash__(self):
    return hash(tuple(sorted(self.items(), key=repr)))


def _to_dict(self):
  """A config's JSON form: its fields without the unset ones (None, empty mappings), nested configs as dicts."""
  return dataclasses.asdict(self, dict_factory=lambda items: {k: dict(v) if isinstance(v, dict) else v
                                                              for k, v in items if v is not None and v != {}})


def foreign_qtyping(meta):
  """Enums and frozen dataclasses with the reference's names, members, fields and defaults -- classes of their own."""
  Q = types.SimpleNamespace(OperatorT=types.SimpleNamespace)

  def field(spec):
    if "required" in spec:
      return dataclasses.field()
    if "enum" in spec:
      return dataclasses.field(default=getattr(Q, spec["enum"])[spec["name"]])
    if "mapping" in spec:
      return dataclasses.field(default_factory=_FrozenMap)
    return dataclasses.field(default=spec["value"])
  for name, members in meta["enums"].items():
    setattr(Q, name, enum.Enum(name, [tuple(m) for m in members], type=str, module=__name__))
  for name, fields in meta["dataclasses"].items():
    setattr(Q, name, dataclasses.make_dataclass(name, [(f, object, field(spec)) for f, spec in fields], frozen=True,
                                                namespace={"to_dict": _to_dict}))
  return Q


@pytest.fixture(scope="module")
def ref():
  with open(os.path.join(GOLDEN, "ref_foreign_objects.json")) as fh:
    meta = json.load(fh)
  with np.load(os.path.join(GOLDEN, "ref_foreign_objects.npz")) as z:
    arrays = {k: z[k] for k in z.files}
  return types.SimpleNamespace(qtyping=foreign_qtyping(meta), meta=meta, arrays=arrays)


def _same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_foreign_objects_are_not_this_packages():
  """The stand-ins must stay foreign: other classes, equal only by value."""
  from mi355q import qtyping as ours
  with open(os.path.join(GOLDEN, "ref_foreign_objects.json")) as fh:
    Q = foreign_qtyping(json.load(fh))
  for name in ("QuantGranularity", "TFLOperationName", "ComputePrecision", "TensorDataType",
               "TensorQuantizationConfig", "OpQuantizationConfig", "OpInfo"):
    assert getattr(Q, name) is not getattr(ours, name), name
  assert Q.QuantGranularity.CHANNELWISE == ours.QuantGranularity.CHANNELWISE
  assert not isinstance(Q.QuantGranularity.CHANNELWISE, ours.QuantGranularity)


@pytest.mark.parametrize("gran", ["TENSORWISE", "CHANNELWISE", "BLOCKWISE_32", "BLOCKWISE_128"])
@pytest.mark.parametrize("bits,symmetric", [(8, True), (8, False), (4, True), (4, False), (16, True)])
def test_zp_scale_from_min_max_takes_the_references_granularity_enum(ref, gran, bits, symmetric):
  from mi355q.algorithms.uniform_quantize import uniform_quantize_tensor as ours
  lo, hi, clips = zp_scale_inputs(gran, bits)
  g_ref = ref.qtyping.QuantGranularity[gran]
  for clip in clips:
    key = zp_scale_key(gran, bits, symmetric, clip)
    want_zp, want_scale = ref.arrays[key + "/zp"], ref.arrays[key + "/scale"]
    got_zp, got_scale = ours.tensor_zp_scale_from_min_max(lo, hi, bits, symmetric, g_ref, clip)      # THEIR enum
    assert _same(got_scale, want_scale) and _same(got_zp, want_zp), (gran, bits, symmetric, clip is None)


@pytest.mark.parametrize("bits,symmetric", [(8, False), (8, True), (16, True)])
def test_activation_quant_params_take_the_references_op_info_and_config(ref, bits, symmetric):
  """The branch with no tensor content (activations: parameters from calibrated min / max) is host arithmetic."""
  from mi355q.algorithms.uniform_quantize import naive_min_max_quantize as ours
  Q = ref.qtyping
  cfg = Q.TensorQuantizationConfig(num_bits=bits, symmetric=symmetric, granularity=Q.QuantGranularity.TENSORWISE)
  info = Q.OpInfo(op=Q.OperatorT(), op_name=Q.TFLOperationName.FULLY_CONNECTED, subgraph_op_index=0,
                  op_quant_config=Q.OpQuantizationConfig(activation_tensor_config=cfg, weight_tensor_config=cfg,
                                                         compute_precision=Q.ComputePrecision.INTEGER))
  qsv = activation_qsv()
  key = activation_key(bits, symmetric)
  want = ref.meta["activation"][key]
  got = ours.get_tensor_quant_params(info, cfg, None, qsv)                                           # THEIR objects
  assert _same(got.scale, ref.arrays[key + "/scale"]) and _same(got.zero_point, ref.arrays[key + "/zero_point"])
  assert (got.num_bits, got.symmetric, got.quantized_dimension, got.block_size) == (
      want["num_bits"], want["symmetric"], want["quantized_dimension"], want["block_size"])
  assert got.quantized_data is None
  with pytest.raises(ValueError) as mine:
    ours.get_tensor_quant_params(info, cfg, None, {"min": qsv["min"]})
  assert str(mine.value) == want["error_without_max"]


def test_qsv_merges_equal_the_references_on_the_same_records(ref):
  from mi355q.utils import qsv_utils as ours
  for i, a, b in qsv_pairs():
    for name in QSV_MERGES:
      got = getattr(ours, name)(dict(a), dict(b))
      assert sorted(got) == ref.meta["qsv_keys"][name], name
      assert all(_same(got[k], ref.arrays[f"qsv/{i}/{name}/{k}"]) for k in got), (i, name)


def test_recipe_manager_takes_the_references_names_and_configs(ref):
  """Scopes added with THEIR op names / configs / algorithm keys resolve like THEIR manager resolves them."""
  from mi355q import recipe_manager as ours
  Q = ref.qtyping
  mine = ours.RecipeManager()
  fill_recipe(mine, Q)
  assert len(ref.meta["recipe"]["resolved"]) == len(RECIPE_LOOKUPS)
  for (scope, op), (scope_t, op_t, alg_t, wt) in zip(RECIPE_LOOKUPS, ref.meta["recipe"]["resolved"]):
    assert (scope, op) == (scope_t, op_t)
    alg_m, cfg_m = mine.get_quantization_configs(Q.TFLOperationName[op], scope)
    assert str(getattr(alg_m, "value", alg_m)) == alg_t, (scope, op)
    wm = cfg_m.weight_tensor_config
    if wt is None:                          # nothing matched: NO_QUANTIZE with an empty config on both sides
      assert wm is None and alg_t == "no_quantize"
      continue
    assert [wm.num_bits, wm.symmetric, str(wm.granularity.value)] == wt, (scope, op)
  # ... and the recipe THEIR manager dumps loads into OURS (the JSON form is the contract between the two)
  theirs = ref.meta["recipe"]["dumped"]
  again = ours.RecipeManager()
  again.load_quantization_recipe(theirs)
  assert json.loads(json.dumps(again.get_quantization_recipe())) == theirs
  assert json.loads(json.dumps(mine.get_quantization_recipe())) == theirs
