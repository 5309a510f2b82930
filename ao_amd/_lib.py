"""ctypes binding of ao_amd/lib/libptv2_hip.so (C ABI: include/ptv2_hip.h).

There is deliberately NO fallback: if the HIP library is missing, fails to load,
or a launcher returns a non-zero status, a RuntimeError is raised.  Nothing in
this package computes on the CPU or through the oracle.
"""
import ctypes
import os
import subprocess

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libptv2_hip.so")
CSRC = os.path.join(_HERE, "csrc")

# name -> (restype, argtypes) of every prototype in include/ptv2_hip.h; pointers are passed as integers (tensor.data_ptr())
_SIGNATURES = _abi.signatures

_ERR = {1: "PTV2_ERR_ARG (invalid argument)", 2: "PTV2_ERR_WORKSPACE (workspace too small)",
        3: "PTV2_ERR_LAUNCH (HIP launch failed)"}
_lib = None
# bumped together with ptv2_abi_version() (ao_amd/csrc/abi.hip) whenever a launcher signature or a struct of
# include/ptv2_hip.h changes (_abi.py derives the ctypes side from the header as it is now; the library holds the header it
# was compiled with): a stale libptv2_hip.so then refuses to load instead of misreading memory
EXPECTED_ABI = 11
# the same for include/ptv2_data_hip.h and ptv2_data_abi_version() (ao_amd/csrc/augment.hip)
EXPECTED_DATA_ABI = 1
# the same for include/ptv2_refine_hip.h and ptv2_refine_abi_version() (ao_amd/csrc/refine.hip)
EXPECTED_REFINE_ABI = 1
# the same for include/ptv2_pp2s_hip.h and ptv2_pp2s_abi_version() (ao_amd/csrc/pp2s.hip)
EXPECTED_PP2S_ABI = 1
# the same for include/ptv2_ptv1_hip.h and ptv2_ptv1_abi_version() (ao_amd/csrc/ptv1.hip)
EXPECTED_PTV1_ABI = 1
# the same for include/ptv2_spconv_hip.h and ptv2_spconv_abi_version() (ao_amd/csrc/spconv_tables.hip)
EXPECTED_SPCONV_ABI = 1
# the same for include/ptv2_pg_hip.h and ptv2_pg_abi_version() (ao_amd/csrc/pointgroup.hip)
EXPECTED_PG_ABI = 1
# the same for include/ptv2_msc_hip.h and ptv2_msc_abi_version() (ao_amd/csrc/msc.hip)
EXPECTED_MSC_ABI = 1
# the same for include/ptv2_st_hip.h and ptv2_st_abi_version() (ao_amd/csrc/stratified.hip)
EXPECTED_ST_ABI = 1
# the same for include/ptv2_inseval_hip.h and ptv2_inseval_abi_version() (ao_amd/csrc/inseval.hip)
EXPECTED_INSEVAL_ABI = 1
# the same for include/ptv2_csc_hip.h and ptv2_csc_abi_version() (ao_amd/csrc/msc_csc.hip)
EXPECTED_CSC_ABI = 1
# the same for include/ptv2_v2m1_hip.h and ptv2_v2m1_abi_version() (ao_amd/csrc/gva_mul.hip)
EXPECTED_V2M1_ABI = 1


def build(verbose=False):
    """Compile every .hip under ao_amd/csrc for gfx950 into ao_amd/lib/libptv2_hip.so (make + hipcc)."""
    cmd = ["make", "-C", CSRC, "-j4", "all"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "ao_amd: %s not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C ao_amd/csrc` (needs hipcc). There is no CPU fallback." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for table in (_SIGNATURES, _abi.data_signatures, _abi.refine_signatures, _abi.pp2s_signatures,
                      _abi.ptv1_signatures, _abi.spconv_signatures, _abi.pg_signatures, _abi.msc_signatures,
                      _abi.st_signatures, _abi.inseval_signatures, _abi.csc_signatures, _abi.v2m1_signatures):
            for name, (res, args) in table.items():
                try:
                    fn = getattr(handle, name)
                except AttributeError:  # a missing symbol is loud by design
                    raise RuntimeError("ao_amd: %s has no `%s` -- stale build; rebuild with `make -C ao_amd/csrc`"
                                       % (LIB_PATH, name)) from None
                fn.restype = res
                fn.argtypes = args
        have = handle.ptv2_abi_version()
        if have != EXPECTED_ABI:
            raise RuntimeError("ao_amd: %s has ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_ABI))
        have = handle.ptv2_data_abi_version()
        if have != EXPECTED_DATA_ABI:
            raise RuntimeError("ao_amd: %s has data ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_DATA_ABI))
        have = handle.ptv2_refine_abi_version()
        if have != EXPECTED_REFINE_ABI:
            raise RuntimeError("ao_amd: %s has refine ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_REFINE_ABI))
        have = handle.ptv2_pp2s_abi_version()
        if have != EXPECTED_PP2S_ABI:
            raise RuntimeError("ao_amd: %s has pp2s ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_PP2S_ABI))
        have = handle.ptv2_ptv1_abi_version()
        if have != EXPECTED_PTV1_ABI:
            raise RuntimeError("ao_amd: %s has ptv1 ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_PTV1_ABI))
        have = handle.ptv2_spconv_abi_version()
        if have != EXPECTED_SPCONV_ABI:
            raise RuntimeError("ao_amd: %s has spconv ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_SPCONV_ABI))
        if handle.ptv2_spconv_struct_bytes(0) != ctypes.sizeof(_abi.spconv_structs["spconv_tables"]):
            raise RuntimeError("ao_amd: spconv_tables is %d bytes in python, %d in %s (stale build)" % (
                ctypes.sizeof(_abi.spconv_structs["spconv_tables"]), handle.ptv2_spconv_struct_bytes(0), LIB_PATH))
        have = handle.ptv2_pg_abi_version()
        if have != EXPECTED_PG_ABI:
            raise RuntimeError("ao_amd: %s has pg ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_PG_ABI))
        if handle.ptv2_pg_struct_bytes(0) != ctypes.sizeof(_abi.pg_structs["pg_csr"]):
            raise RuntimeError("ao_amd: pg_csr is %d bytes in python, %d in %s (stale build)" % (
                ctypes.sizeof(_abi.pg_structs["pg_csr"]), handle.ptv2_pg_struct_bytes(0), LIB_PATH))
        have = handle.ptv2_msc_abi_version()
        if have != EXPECTED_MSC_ABI:
            raise RuntimeError("ao_amd: %s has msc ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_MSC_ABI))
        have = handle.ptv2_st_abi_version()
        if have != EXPECTED_ST_ABI:
            raise RuntimeError("ao_amd: %s has st ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_ST_ABI))
        if handle.ptv2_st_struct_bytes(0) != ctypes.sizeof(_abi.st_structs["st_args"]):
            raise RuntimeError("ao_amd: st_args is %d bytes in python, %d in %s (stale build)" % (
                ctypes.sizeof(_abi.st_structs["st_args"]), handle.ptv2_st_struct_bytes(0), LIB_PATH))
        have = handle.ptv2_inseval_abi_version()
        if have != EXPECTED_INSEVAL_ABI:
            raise RuntimeError("ao_amd: %s has inseval ABI version %d, the python side expects %d -- stale build; rebuild "
                               "with `make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_INSEVAL_ABI))
        have = handle.ptv2_csc_abi_version()
        if have != EXPECTED_CSC_ABI:
            raise RuntimeError("ao_amd: %s has csc ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_CSC_ABI))
        have = handle.ptv2_v2m1_abi_version()
        if have != EXPECTED_V2M1_ABI:
            raise RuntimeError("ao_amd: %s has v2m1 ABI version %d, the python side expects %d -- stale build; rebuild with "
                               "`make -C ao_amd/csrc`" % (LIB_PATH, have, EXPECTED_V2M1_ABI))
        for which, name in enumerate(("ptv1_params", "ptv1_norms", "ptv1_grads")):
            if handle.ptv2_ptv1_struct_bytes(which) != ctypes.sizeof(_abi.ptv1_structs[name]):
                raise RuntimeError("ao_amd: %s is %d bytes in python, %d in %s (stale build)" % (
                    name, ctypes.sizeof(_abi.ptv1_structs[name]), handle.ptv2_ptv1_struct_bytes(which), LIB_PATH))
        for which, name in enumerate(("ptv2_aug_step", "ptv2_aug_program")):
            if handle.ptv2_data_struct_bytes(which) != ctypes.sizeof(_abi.data_structs[name]):
                raise RuntimeError("ao_amd: %s is %d bytes in python, %d in %s (stale build)" % (
                    name, ctypes.sizeof(_abi.data_structs[name]), handle.ptv2_data_struct_bytes(which), LIB_PATH))
        _lib = handle
    return _lib


def check_struct(which, mirror):
    """A ctypes mirror of a C struct must have the size the library was compiled with."""
    have, want = lib().ptv2_struct_bytes(which), ctypes.sizeof(mirror)
    if have != want:
        raise RuntimeError("ao_amd: %s is %d bytes in python, %d in %s (stale build or a drifted mirror)"
                           % (mirror.__name__, want, have, LIB_PATH))


def check(status, what):
    if status != 0:
        raise RuntimeError("ao_amd: %s failed with status %d: %s" % (what, status, _ERR.get(status, "?")))


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("ao_amd ops run on the GPU only (got a %s tensor); there is no CPU fallback" % t.device)


def ptr(t):
    return 0 if t is None else t.data_ptr()


_WS = {}


def workspace(nbytes, device):
    """Scratch for one launcher call.  One grow-only buffer per (device, stream): launches on a stream are
    ordered, and no launcher needs its scratch after it returns, so consecutive calls can share it (saves an
    allocator round trip per op; at 288 GB per GPU the retained high-water mark is irrelevant)."""
    nbytes = max(int(nbytes), 256)
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def kernel_timer(enable, only=None, stride=1):
    """Switch the in-library per-kernel HIP-event timer (include/ptv2_hip.h: ptv2_profile_*).  `only` = kernel
    name: bracket that kernel alone (a whole-step measurement is then not perturbed by ~2000 event pairs)."""
    L = lib()
    kid = -1
    if only is not None:
        name = ctypes.create_string_buffer(64)
        us, cnt, byt = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        for i in range(L.ptv2_profile_kernel_count()):
            L.ptv2_profile_read(i, name, ctypes.byref(us), ctypes.byref(cnt), ctypes.byref(byt))
            if name.value.decode() == only:
                kid = i
        if kid < 0:
            raise ValueError("unknown kernel name %r" % only)
    L.ptv2_profile_select(kid)
    L.ptv2_profile_stride(int(stride))
    L.ptv2_profile_enable(1 if enable else 0)


def graph_stats(reset=False):
    """Counters of the graph-issued model launchers (ao_amd/csrc/graph.hip)."""
    out = (ctypes.c_double * 9)()
    lib().ptv2_graph_stats(out, 1 if reset else 0)
    keys = ("scopes", "updated", "instantiated", "declined", "nodes", "capture_us", "update_us", "launch_us", "wait_us")
    return dict(zip(keys, [float(v) for v in out]))


def kernel_timer_read():
    """{kernel name: dict(launches, total_us, avg_us, bytes_per_launch)} for kernels launched while enabled."""
    L = lib()
    out = {}
    name = ctypes.create_string_buffer(64)
    us, cnt, byt = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
    for kid in range(L.ptv2_profile_kernel_count()):
        if L.ptv2_profile_read(kid, name, ctypes.byref(us), ctypes.byref(cnt), ctypes.byref(byt)) == 0 and cnt.value > 0:
            out[name.value.decode()] = dict(launches=cnt.value, total_us=us.value, avg_us=us.value / cnt.value,
                                            bytes_per_launch=byt.value)
    return out
