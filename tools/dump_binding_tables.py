#!/usr/bin/env python
"""Prints what the binding tells ctypes about libgnn_hip.so, in a canonical text form: per function the return type and the
argument types, per struct every field with type, offset and size, per constant its value.  Uses the public names of
gnn_fpga_amd._lib only, so it runs on any commit; two commits bind the same ABI when their outputs are equal
(profiles/binding_tables_ab.txt).  Needs neither the library nor a GPU.

    python tools/dump_binding_tables.py [REPO] > tables.txt
"""
import ctypes
import importlib
import os
import sys

sys.path.insert(0, os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..")))
from gnn_fpga_amd import _lib  # noqa: E402

# the header constants every commit's _lib has under these names (the dictionaries carry header values under Python keys)
CONSTANTS = ("GNN_ABI_VERSION", "GNN_ERR_UNSUPPORTED", "GNN_ERR_BADARG", "GNN_ERR_WORKSPACE", "GNN_FLAG_EXP_PRODUCT",
             "GNN_FLAG_BF16_MLP", "GNN_GCN_MAX_LAYERS", "GNN_ITER_MAX", "GNN_FX_STAGES", "GNN_FX_ROUNDING",
             "GNN_FX_OVERFLOW", "GNN_TOY_SEGMENTS", "GNN_TOY_HITS", "GNN_TOY_NORMS", "TRACKS_MODES",
             "SELECT_HITS_MAX_LAYERS", "ROUTE_FIELDS", "ROUTE_NAMES")


def type_name(t):
    if t is None:
        return "None"
    if issubclass(t, ctypes.Array):
        return "%s[%d]" % (type_name(t._type_), t._length_)
    if issubclass(t, ctypes._Pointer):
        return "POINTER(%s)" % type_name(t._type_)
    return t.__name__


for table in ("SIGNATURES", "ITER_SIGNATURES", "FX_SIGNATURES", "FXEV_SIGNATURES"):
    for name, (res, args) in sorted(getattr(_lib, table).items()):
        print("%s %s: %s (%s)" % (table, name, type_name(res), ", ".join(map(type_name, args))))
for name, cls in sorted(vars(_lib).items()):
    if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure:
        print("struct %s sizeof %d" % (name, ctypes.sizeof(cls)))
        for field, t in cls._fields_:
            print("  %s %s offset %d size %d" % (field, type_name(t), getattr(cls, field).offset, getattr(cls, field).size))
for name in CONSTANTS:
    print("constant %s = %r" % (name, getattr(_lib, name)))
print("constant select_hits.MAX_LAYERS = %r" % importlib.import_module("gnn_fpga_amd.select_hits").MAX_LAYERS)
