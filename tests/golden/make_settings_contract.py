#!/usr/bin/env python3
"""Generate tests/golden/settings_contract.json — what rfwhip_set_setting / rfwhip_get_setting / rfwhip_get_settings answer, as
recorded from the host-emulation library (tests/emu/build_emu.py) of the commit BEFORE the settings became one table.
tests/test_settings_contract.py holds every later library to it entry for entry (strings and integers: no tolerance).

Probes, each on a fresh context, once as created and once after rfwhip_init(16, 16):
  keys      rfwhip_get_settings
  defaults  rfwhip_get_setting of every listed key, of the retired "arm", of the read-only keys and of "no_such_key"
  sets      per key: rfwhip_set_setting of every value of VALUES in order on ONE context, each followed by a get
A get is recorded as [code, value or error text], a set as [code, error text or "", the get that follows].

    python tests/golden/make_settings_contract.py [library]      (default: the emulation library of this tree)
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "settings_contract.json")
UNLISTED = ["arm", "shadow_packets_on", "shadow_bins_per_run", "textured", "packet", "world_tree", "sky", "no_such_key"]
VALUES = ["0", "1", "2", "-1", "-2", "3", "15", "16", "64", "65", "4096", "4097", "0.5", "1", "1.5", "1e31", "nan", "", "abc",
          "pt", "parity", "xor128", "center", "host", "device", "hash", "bluenoise", "bogus"]
STATES = ("created", "initialised")


def declare(lib):
    vp, i32 = C.c_void_p, C.c_int
    for name, res, args in [("create", i32, [i32, i32, i32, C.POINTER(vp)]), ("destroy", None, [vp]),
                            ("init", i32, [vp, C.c_uint32, C.c_uint32]), ("last_error", C.c_char_p, []),
                            ("set_setting", i32, [vp, C.c_char_p, C.c_char_p]),
                            ("get_setting", i32, [vp, C.c_char_p, C.c_char_p, C.c_size_t]),
                            ("get_settings", i32, [vp, C.POINTER(C.c_char_p), C.c_size_t])]:
        f = getattr(lib, "rfwhip_" + name)
        f.restype, f.argtypes = res, args


class Fresh:
    """A context of its own for one probe."""

    def __init__(self, lib, state):
        self.lib, self.ctx = lib, C.c_void_p()
        assert lib.rfwhip_create(0, 0, 1, C.byref(self.ctx)) == 0
        if state == "initialised":
            assert lib.rfwhip_init(self.ctx, 16, 16) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.rfwhip_destroy(self.ctx)

    def error(self):
        return (self.lib.rfwhip_last_error() or b"").decode(errors="replace")

    def keys(self):
        keys = (C.c_char_p * 256)()
        n = self.lib.rfwhip_get_settings(self.ctx, keys, 256)
        return [keys[i].decode() for i in range(n)]

    def get(self, key):
        buf = C.create_string_buffer(256)
        rc = self.lib.rfwhip_get_setting(self.ctx, key.encode(), buf, 256)
        return [rc, self.error() if rc else buf.value.decode()]

    def set(self, key, value):
        rc = self.lib.rfwhip_set_setting(self.ctx, key.encode(), value.encode())
        return [rc, self.error() if rc else "", self.get(key)]


def probe_keys(lib, state):
    with Fresh(lib, state) as c:
        return c.keys()


def probe_defaults(lib, state, keys):
    with Fresh(lib, state) as c:
        return {k: c.get(k) for k in keys}


def probe_sets(lib, state, key):
    with Fresh(lib, state) as c:
        return [c.set(key, v) for v in VALUES]


def record(lib):
    declare(lib)
    out = {"values": VALUES}
    for state in STATES:
        listed = probe_keys(lib, state)
        keys = listed + UNLISTED
        out[state] = {"keys": listed, "defaults": probe_defaults(lib, state, keys),
                      "sets": {k: probe_sets(lib, state, k) for k in keys}}
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        sys.path.insert(0, os.path.join(os.path.dirname(HERE), "emu"))
        import build_emu
        path = build_emu.build()
    rec = record(C.CDLL(path))
    with open(OUT, "w") as f:  # one line per key: a changed answer shows as a one-line diff
        f.write("{\n")
        f.write(' "values": %s,\n' % json.dumps(rec["values"]))
        for si, state in enumerate(STATES):
            r = rec[state]
            f.write(' "%s": {\n  "keys": %s,\n' % (state, json.dumps(r["keys"])))
            for part in ("defaults", "sets"):
                rows = ['   %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in r[part].items()]
                f.write('  "%s": {\n%s\n  }%s\n' % (part, ",\n".join(rows), "," if part == "defaults" else ""))
            f.write(" }%s\n" % ("," if si == 0 else ""))
        f.write("}\n")
    print(OUT, os.path.getsize(OUT), "bytes")
