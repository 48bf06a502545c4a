"""Phasing heterozygous sites from reads restated over dicts and sorted lists ("Phasing heterozygous sites from reads" in
include/classpro_amd.h): a table P is [(key, count)] of canonical K-mers ascending, key = the bases as a 2K-bit number,
first base most significant; reads are bytes.  Imports nothing of the product."""
import hetpairs_oracle as HO

CODE = {65: 0, 67: 1, 71: 2, 84: 3}
TALLY = ("edges", "kept", "tied", "weak", "forest", "conflicts", "blocks", "single", "largest", "rounds", "bad")


def encode(s):
    x = 0
    for c in s:
        x = x * 4 + CODE[c]
    return x


def decode(x, K):
    return bytes(b"ACGT"[(x >> (2 * (K - 1 - p))) & 3] for p in range(K))


def revcomp_seq(s):
    return bytes({65: 84, 67: 71, 71: 67, 84: 65}.get(c, c) for c in reversed(s))


def kmers(s, K, canonical=True):
    """(j, key) for every K-mer s[j:j+K] of upper-case A C G T, the key rolled base by base."""
    mask, top, fw, rc, valid = (1 << 2 * K) - 1, 2 * K - 2, 0, 0, 0
    for i, c in enumerate(s):
        b = CODE.get(c)
        if b is None:
            fw = rc = valid = 0
            continue
        fw, rc, valid = (fw << 2 | b) & mask, rc >> 2 | (3 - b) << top, valid + 1
        if valid >= K:
            yield i - K + 1, min(fw, rc) if canonical else fw


def table(seqs, K, canonical=True):
    """The count table of the k-mers of upper-case A C G T of `seqs`, ascending."""
    cnt = {}
    for s in seqs:
        for _, x in kmers(s, K, canonical):
            cnt[x] = cnt.get(x, 0) + 1
    return sorted(cnt.items())


def sites(P, K):
    """(mate, mark, nsites) of the entries of P: siblings inside P with no range."""
    sib = HO.siblings(P, K)
    at = {x: i for i, (x, _) in enumerate(P)}
    mate = []
    for x, _ in P:
        ys = sib[x]
        y = next(iter(ys)) if len(ys) == 1 else None
        mate.append(at[y] if y is not None and len(sib[y]) == 1 else -1)
    mark, ns = [-1] * len(P), 0
    for i, m in enumerate(mate):
        if m > i:
            mark[i], mark[m] = ns << 1, ns << 1 | 1
            ns += 1
    return mate, mark, ns


def link_key(s, a, s2, a2):
    return min(s, s2) << 32 | max(s, s2) << 1 | (a ^ a2)


def read_links(P, mark, reads, K, canonical=True):
    """(links in batch order, [markers, links, self])"""
    at = {x: i for i, (x, _) in enumerate(P)}
    links, nmark, nself = [], 0, 0
    for s in reads:
        prev = None
        for _, x in kmers(s, K, canonical):
            i = at.get(x)
            if i is None or mark[i] < 0:
                continue
            nmark += 1
            cur = (mark[i] >> 1, mark[i] & 1)
            if prev is not None:
                if prev[0] == cur[0]:
                    nself += 1
                else:
                    links.append(link_key(prev[0], prev[1], cur[0], cur[1]))
            prev = cur
    return links, [nmark, len(links), nself]


def forest(counts, nsites, min_support=2):
    """counts: {link key: occurrences}.  Returns (block, side, tally dict): Kruskal over the kept edges from first to last;
    `rounds` are the Boruvka rounds that join trees, counted over the same order."""
    t = dict.fromkeys(TALLY, 0)
    pair = {}
    for key, c in counts.items():
        s, u = key >> 32, (key & 0xFFFFFFFF) >> 1
        if key >> 63 or s >= u or u >= nsites:
            t["bad"] += 1
            continue
        pair.setdefault((s, u), [0, 0])[key & 1] += c
    kept = []
    for (s, u), (cis, trans) in sorted(pair.items()):
        t["edges"] += 1
        w, l = max(cis, trans), min(cis, trans)
        if w < min_support:
            t["weak"] += 1
        elif w == l:
            t["tied"] += 1
        else:
            t["kept"] += 1
            kept.append((-min(w - l, 65535), s, u, int(trans > cis)))
    kept.sort()
    parent = list(range(nsites))

    def find(p, v):
        while p[v] != v:
            p[v] = p[p[v]]
            v = p[v]
        return v

    adj = [[] for _ in range(nsites)]
    for _, s, u, sign in kept:
        a, b = find(parent, s), find(parent, u)
        if a != b:
            parent[a] = b
            adj[s].append((u, sign))
            adj[u].append((s, sign))
            t["forest"] += 1
    block, side = list(range(nsites)), [0] * nsites
    seen = [False] * nsites
    for r in range(nsites):                                # ascending: the first site of a tree met is its smallest
        if seen[r]:
            continue
        seen[r], todo, size = True, [r], 1
        while todo:
            v = todo.pop()
            for u, sign in adj[v]:
                if not seen[u]:
                    seen[u], block[u], side[u] = True, r, side[v] ^ sign
                    size += 1
                    todo.append(u)
        if size >= 2:
            t["blocks"] += 1
            t["largest"] = max(t["largest"], size)
        else:
            t["single"] += 1
    t["conflicts"] = sum(sign != side[s] ^ side[u] for _, s, u, sign in kept)
    comp = list(range(nsites))                             # the rounds: every tree takes its first edge that leaves it
    while True:
        best = {}
        for e in kept:
            a, b = find(comp, e[1]), find(comp, e[2])
            if a != b:
                for r in (a, b):
                    if r not in best or e < best[r]:
                        best[r] = e
        if not best:
            break
        for e in best.values():
            a, b = find(comp, e[1]), find(comp, e[2])
            if a != b:
                comp[a] = b
        t["rounds"] += 1
    return block, side, t


def split(P, mark, block, side):
    """(A, B) as [(key, count)]"""
    linked = [False] * len(block)
    for s, b in enumerate(block):
        if b != s:
            linked[s] = linked[b] = True
    out = ([], [])
    for (x, c), m in zip(P, mark):
        if m >= 0 and linked[m >> 1]:
            out[side[m >> 1] ^ (m & 1)].append((x, c))
    return out


def phase(T, K, batches, count_range=None, min_support=2):
    """The driver over a table T and batches of reads: a dict as SortedKmers.phase returns, tables as [(key, count)]."""
    P = HO.members(T, K, count_range, True)
    mate, mark, ns = sites(P, K)
    counts, lt = {}, [0, 0, 0]
    for reads in batches:
        links, t = read_links(P, mark, reads, K)
        lt = [a + b for a, b in zip(lt, t)]
        for k in links:
            counts[k] = counts.get(k, 0) + 1
    block, side, ft = forest(counts, ns, min_support)
    A, B = split(P, mark, block, side)
    return {"P": P, "A": A, "B": B, "mate": mate, "mark": mark, "block": block, "side": side, "nsites": ns,
            "sites": {"mated": 2 * ns, "unmated": len(P) - 2 * ns}, "links": dict(zip(("markers", "links", "self"), lt)),
            "forest": ft}


def lines(r, nseqs):
    f = r["forest"]
    return ("tabphase: %d k-mers, %d sites, %d sequences, %d markers, %d links, %d self\n"
            % (len(r["P"]), r["nsites"], nseqs, r["links"]["markers"], r["links"]["links"], r["links"]["self"]),
            "tabphase: %d edges, %d kept, %d tied, %d weak, %d conflicts, %d blocks, largest %d sites, %d unlinked sites\n"
            % (f["edges"], f["kept"], f["tied"], f["weak"], f["conflicts"], f["blocks"], f["largest"], f["single"]))


def sites_tsv(r, K):
    P, mate, block, side = r["P"], r["mate"], r["block"], r["side"]
    linked = [False] * r["nsites"]
    for s, b in enumerate(block):
        if b != s:
            linked[s] = linked[b] = True
    rows, s = [], 0
    for i, m in enumerate(mate):
        if m > i:
            rows.append(b"%d\t%d\t%d\t%s\t%s\t%d\t%d\n" % (s, block[s] if linked[s] else -1, side[s], decode(P[i][0], K),
                                                        decode(P[m][0], K), P[i][1], P[m][1]))
            s += 1
    return b"".join(rows)


def genome(rng, K, length=30000, gap=(60, 140), edge=500):
    """Two haplotypes that differ by SNPs more than K apart and more than `edge` + K from the ends, where reads tiled every
    `edge` bases begin to overlap: (h1, h2, SNP positions)."""
    h1 = bytearray(rng.choice(b"ACGT") for _ in range(length))
    h2, snps, p = bytearray(h1), [], edge + K + 1 + rng.randint(*gap)
    while p < length - edge - K - 1:
        h2[p] = rng.choice([c for c in b"ACGT" if c != h1[p]])
        snps.append(p)
        p += K + 1 + rng.randint(*gap)
    return bytes(h1), bytes(h2), snps


def tiled_reads(haps, rlen=3000, step=500):
    """Error-free reads of rlen bases every `step` bases over every haplotype, every second one reverse-complemented."""
    out = []
    for h in haps:
        for k, a in enumerate(range(0, len(h) - rlen + 1, step)):
            out.append(revcomp_seq(h[a:a + rlen]) if k & 1 else h[a:a + rlen])
    return out
