#!/usr/bin/env python3
"""Record the fixtures of tests/test_reference_objects.py by running the REAL reference.

Usage (wherever a copy of the reference exists; the tests themselves never need it):
    python tests/golden/gen/make_foreign_objects_golden.py <path of the reference's ai_edge_quantizer package>

The reference's modules are imported unmodified, the same way make_golden.py does it (an empty package object whose
__path__ is the reference directory, tests/golden/gen/shim/ first on sys.path), and the same calls the tests make are
made on the reference's own objects. Written:
    tests/golden/ref_foreign_objects.json  the reference's enum members and dataclass fields (names, values, defaults:
                                           what the tests build their foreign objects from) and the scalar results
    tests/golden/ref_foreign_objects.npz   the array results, keyed as the tests look them up
Nothing from the reference is copied: fixtures are names, inputs' seeds and outputs only.
"""
import dataclasses
import enum
import json
import os
import sys
sys.dont_write_bytecode = True  # never leave .pyc files in the reference tree
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
TESTS = os.path.dirname(GOLDEN)
ENUMS = ("QuantGranularity", "TFLOperationName", "ComputePrecision", "TensorDataType")
DATACLASSES = ("TensorQuantizationConfig", "OpQuantizationConfig", "OpInfo")


def bootstrap(ref_dir):
  sys.path.insert(0, os.path.join(HERE, "shim"))
  pkg = types.ModuleType("ai_edge_quantizer")
  pkg.__path__ = [ref_dir]
  sys.modules["ai_edge_quantizer"] = pkg


def encode_default(f):
  """One dataclass field's default, as the tests decode it (tests/test_reference_objects.py: _default)."""
  if f.default is not dataclasses.MISSING:
    v = f.default
    if isinstance(v, enum.Enum):
      return {"enum": type(v).__name__, "name": v.name}
    if v is None or isinstance(v, (bool, int, float, str)):
      return {"value": v}
    raise TypeError(f"{f.name}: default {v!r} has no encoding")
  if f.default_factory is not dataclasses.MISSING:
    v = f.default_factory()
    if hasattr(v, "keys") and not len(v):
      return {"mapping": {}}
    raise TypeError(f"{f.name}: default factory gives {v!r}")
  return {"required": True}


def main():
  if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
    raise SystemExit(__doc__)
  bootstrap(os.path.abspath(sys.argv[1]))
  sys.path.insert(0, TESTS)
  import ml_dtypes  # the shim  # noqa: F401
  from ai_edge_quantizer import qtyping as Q, recipe_manager
  from ai_edge_quantizer.algorithms.uniform_quantize import naive_min_max_quantize as mm
  from ai_edge_quantizer.algorithms.uniform_quantize import uniform_quantize_tensor as uqt
  from ai_edge_quantizer.utils import qsv_utils
  import test_reference_objects as T     # the cases: inputs are made by the same functions the tests call

  meta = {"enums": {n: [[m.name, m.value] for m in getattr(Q, n)] for n in ENUMS},
          "dataclasses": {n: [[f.name, encode_default(f)] for f in dataclasses.fields(getattr(Q, n))] for n in DATACLASSES}}
  arr = {}
  # ---- tensor_zp_scale_from_min_max
  for gran, bits, symmetric in T.ZP_SCALE_CASES:
    lo, hi, clips = T.zp_scale_inputs(gran, bits)
    aware = (lambda a: a.view(ml_dtypes.Bf16Aware)) if gran.startswith("BLOCKWISE") else (lambda a: a)
    for clip in clips:
      zp, scale = uqt.tensor_zp_scale_from_min_max(aware(lo), aware(hi), bits, symmetric, Q.QuantGranularity[gran], clip)
      key = T.zp_scale_key(gran, bits, symmetric, clip)
      arr[key + "/zp"], arr[key + "/scale"] = np.asarray(zp).view(np.ndarray), np.asarray(scale).view(np.ndarray)
  # ---- the activation branch of get_tensor_quant_params
  meta["activation"] = {}
  for bits, symmetric in T.ACTIVATION_CASES:
    cfg = Q.TensorQuantizationConfig(num_bits=bits, symmetric=symmetric, granularity=Q.QuantGranularity.TENSORWISE)
    info = Q.OpInfo(op=Q.OperatorT(), op_name=Q.TFLOperationName.FULLY_CONNECTED, subgraph_op_index=0,
                    op_quant_config=Q.OpQuantizationConfig(activation_tensor_config=cfg, weight_tensor_config=cfg,
                                                           compute_precision=Q.ComputePrecision.INTEGER))
    qsv = T.activation_qsv()
    p = mm.get_tensor_quant_params(info, cfg, None, qsv)
    assert p.quantized_data is None
    key = T.activation_key(bits, symmetric)
    arr[key + "/scale"], arr[key + "/zero_point"] = np.asarray(p.scale), np.asarray(p.zero_point)
    try:
      mm.get_tensor_quant_params(info, cfg, None, {"min": qsv["min"]})
      raise AssertionError("the reference accepted a QSV without max")
    except ValueError as e:
      error = str(e)
    meta["activation"][key] = {"num_bits": p.num_bits, "symmetric": p.symmetric,
                               "quantized_dimension": p.quantized_dimension, "block_size": p.block_size,
                               "error_without_max": error}
  # ---- QSV merges
  for i, a, b in T.qsv_pairs():
    for name in T.QSV_MERGES:
      got = getattr(qsv_utils, name)(dict(a), dict(b))
      meta.setdefault("qsv_keys", {})[name] = sorted(got)
      for k, v in got.items():
        arr[f"qsv/{i}/{name}/{k}"] = np.asarray(v)
  # ---- recipe manager
  rm = recipe_manager.RecipeManager()
  T.fill_recipe(rm, Q)
  resolved = []
  for scope, op in T.RECIPE_LOOKUPS:
    alg, cfg = rm.get_quantization_configs(Q.TFLOperationName[op], scope)
    w = cfg.weight_tensor_config
    resolved.append([scope, op, str(getattr(alg, "value", alg)),
                     None if w is None else [w.num_bits, w.symmetric, str(w.granularity.value)]])
  meta["recipe"] = {"resolved": resolved, "dumped": json.loads(json.dumps(rm.get_quantization_recipe()))}

  with open(os.path.join(GOLDEN, "ref_foreign_objects.json"), "w") as fh:
    json.dump(meta, fh, indent=1)
    fh.write("\n")
  np.savez_compressed(os.path.join(GOLDEN, "ref_foreign_objects.npz"), **arr)
  print(f"{len(arr)} arrays, {len(resolved)} recipe lookups")


if __name__ == "__main__":
  main()
