#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libcmpc.so: every function
symbol of every code object (kernel_hash.py's bundle and symbol walk), its
size and the sha256 of its machine code.  A host-only change must leave the
symbol sets, sizes and hashes equal.

usage: kernel_hash_diff.py OLD.so NEW.so     (exit status 1 on any difference)"""
import hashlib
import struct
import sys

from kernel_hash import _sections, code_objects


def functions(path):
    """{symbol: (size, sha256)} over the gfx950 code objects of path."""
    out = {}
    for co in code_objects(open(path, "rb").read()):
        secs, hdrs = _sections(co)
        if ".symtab" not in secs:
            continue
        off, size, _, _, link, entsize = secs[".symtab"]
        stroff = hdrs[link][3]
        for k in range(size // entsize):
            name, info, other, shndx, value, sz = struct.unpack_from("<IBBHQQ", co, off + k * entsize)
            if (info & 0xF) != 2 or not sz:  # STT_FUNC
                continue
            sym = co[stroff + name:co.index(b"\0", stroff + name)].decode()
            sh = hdrs[shndx]
            faddr = sh[3] + (value - sh[2])
            out[sym] = (sz, hashlib.sha256(co[faddr:faddr + sz]).hexdigest())
    return out


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    changed = sorted(s for s in set(old) & set(new) if old[s] != new[s])
    for tag, syms in (("only in old", gone), ("only in new", added)):
        for s in syms:
            print(f"{tag}: {s}")
    for s in changed:
        print(f"differs: {s}  {old[s][0]} B {old[s][1][:16]} -> {new[s][0]} B {new[s][1][:16]}")
    print(f"{len(old)} symbols in old, {len(new)} in new: {len(gone)} removed, {len(added)} added, "
          f"{len(changed)} changed")
    return 1 if gone or added or changed else 0


if __name__ == "__main__":
    sys.exit(main())
