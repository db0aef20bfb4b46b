"""numpy model of vidc_rebalance_sharded (include/vidc.h): the new owner of every list is lpt_partition of the object's CURRENT sizes, the
local number of a list is its rank among its owner's lists, and every new shard gets one (old shard, old local number) row per local
list -- the table vidc_roc_regroup takes.  moved_ids = the ids whose owner changes.  Also the batches the re-balance tests skew family F
with (tests/test_shards_cpu.py: F_SIZES)."""
import numpy as np

NLIST, NTOTAL = 37, 15404


def local_numbers(owner, ns):
    owner = np.asarray(owner, np.int64)
    local = np.zeros(owner.size, np.int64)
    lists = []
    for s in range(ns):
        mine = np.nonzero(owner == s)[0]
        local[mine] = np.arange(mine.size)
        lists.append(mine)
    return local, lists


class Rebalance:
    """sizes: the lists' current sizes; old_owner: the map they sit under -> new_owner, both local numberings, rows[d] = (src_no,
    list_no) per new shard, loads of the new map, moved_ids"""

    def __init__(self, sizes, ns, old_owner):
        from vector_db_id_compression_amd.sharding import lpt_partition

        self.sizes = np.asarray(sizes, np.int64)
        self.ns = ns
        self.old_owner = np.asarray(old_owner, np.int64)
        self.new_owner = lpt_partition(self.sizes, ns).astype(np.int64)
        self.old_local, self.old_lists = local_numbers(self.old_owner, ns)
        self.new_local, self.new_lists = local_numbers(self.new_owner, ns)
        self.rows = [(self.old_owner[mine], self.old_local[mine]) for mine in self.new_lists]
        self.loads = np.bincount(self.new_owner, weights=self.sizes, minlength=ns).astype(np.int64)[:ns]
        self.moved_ids = int(self.sizes[self.old_owner != self.new_owner].sum())

    def arrivals_and_departures(self):
        """per shard: lists that arrive at it and lists that leave it"""
        changed = self.old_owner != self.new_owner
        arrive = np.bincount(self.new_owner[changed], minlength=self.ns)
        leave = np.bincount(self.old_owner[changed], minlength=self.ns)
        return arrive, leave


def f_owner(ns):
    """the map family F is encoded under"""
    from vector_db_id_compression_amd.sharding import lpt_partition

    from test_shards_cpu import F_SIZES

    return lpt_partition(np.asarray(F_SIZES, np.int64), ns).astype(np.int64)


def skew_shard(ns):
    """the shard that owns the most lists of family F (the lowest such): at 8 shards shard 0 owns the 3000-id list alone, and growing
    that list leaves the map as it is"""
    return int(np.argmax(np.bincount(f_owner(ns), minlength=ns)))


def skew_batch(ns, n=900, seed=23):
    """n (list, id) pairs into the lists ONE shard owns at ns shards (skew_shard; empty lists included), interleaved; the ids are new,
    distinct and below 2^14, the packed width of family F"""
    mine = np.nonzero(f_owner(ns) == skew_shard(ns))[0]
    rng = np.random.default_rng(seed + ns)
    ln = mine[rng.integers(0, mine.size, n)].astype(np.int64)
    ids = (NTOTAL + rng.permutation(n)).astype(np.uint64)
    assert int(ids.max()) < 2 ** 14
    return ln, ids


def second_batch(n=80, seed=29):
    """a batch for every list, behind the skew batch: ids 16 304 .. 16 383, still below 2^14"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, NLIST, n).astype(np.int64), (NTOTAL + 900 + rng.permutation(n)).astype(np.uint64)


def grown_sizes(ns, n=900, seed=23):
    from test_shards_cpu import F_SIZES

    ln, _ = skew_batch(ns, n, seed)
    return np.asarray(F_SIZES, np.int64) + np.bincount(ln, minlength=NLIST)


def remove_batch(off, ids, ns):
    """every third id of the lists shard 0 owns at ns shards, as (list, id) pairs"""
    off = np.asarray(off, np.int64)
    ln, out = [], []
    for l in np.nonzero(f_owner(ns) == 0)[0]:
        part = ids[off[l]: off[l + 1]][::3]
        ln.append(np.full(part.size, l, np.int64))
        out.append(part)
    return np.concatenate(ln), np.concatenate(out).astype(np.uint64)


def shrunk_sizes(off, ns):
    from test_shards_cpu import F_SIZES

    sizes = np.asarray(F_SIZES, np.int64).copy()
    mine = f_owner(ns) == 0
    sizes[mine] -= (sizes[mine] + 2) // 3
    return sizes
