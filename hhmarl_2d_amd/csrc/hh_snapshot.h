/*
 * hh_snapshot.h — opaque, complete, versioned snapshots of a world, a policy bank and a commander net (C ABI: hh_world_snapshot* in
 * include/hh_abi.h, hh_policy_snapshot* in include/hh_policy.h, hh_commander_snapshot* in include/hh_commander.h).
 *
 * Copies only: no kernel, no launch.  A blob is [host] memory:
 *     HhSnapHeader (208 bytes) | section 0 | section 1 | ...      every section starts on a 16-byte boundary
 * world:     0 the creating hh_config | 1 the world's device slab (every array of DevPtrs that lives in it, the event masks, the
 *            macro-step counter words with hh_hl_tick_count's counter) | 2 the bound bank's row counters | 3 its row lists (2 and 3 are
 *            empty for a world without a bound bank)
 * bank:      0 the selector LUT [256] | 1 the row counters | 2 the row lists | 3 + s: slot s as the kernels read it — fp32 blob, fp16
 *            planes, fragment stream, then the value branch's planes + biases and its fragment stream (HH_POLICY_PART_* order; empty
 *            for an empty slot)
 * commander: 0 the packed weights (fp16 planes, then the fp32 section)
 * The header's aux words: world — [0] max_rows of the bound bank (0: none); bank — [0] n_rows of the call that built the row lists,
 * [1 + s] slot s: -1 empty, else kind | 16 when the value branch is loaded; commander — [0] weights loaded.
 * A restore checks magic, version, digest, N, A, slots, aux and every section size against the receiving object BEFORE it writes.
 */
#ifndef HH_SNAPSHOT_H
#define HH_SNAPSHOT_H

#define HH_SNAP_MAGIC_WORLD 0x57534848u     /* "HHSW" */
#define HH_SNAP_MAGIC_POLICY 0x50534848u    /* "HHSP" */
#define HH_SNAP_MAGIC_COMMANDER 0x43534848u /* "HHSC" */
#define HH_SNAP_VERSION 1u
#define HH_SNAP_MAX_SECTIONS 16
#define HH_SNAP_AUX 12

struct HhSnapHeader {
    uint32_t magic, version;
    uint64_t digest;                 /* FNV-1a of the creating hh_config (world) / of the geometry words (bank, commander) */
    int32_t N, A, slots, n_sections; /* world: arenas, unit slots, 0; bank: max_rows, 0, HH_POLICY_MAX_NETS; commander: 0, HH_CMD_AGENTS, 1 */
    int32_t aux[HH_SNAP_AUX];
    uint64_t section_bytes[HH_SNAP_MAX_SECTIONS];
};
static_assert(sizeof(HhSnapHeader) == 208, "snapshot header layout");

struct HhSnapSection { void *dev; size_t bytes; const void *host; }; /* dev: a device range, or host: a host range (dev == nullptr) */

static uint64_t hh_snap_fnv(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ULL) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ULL; }
    return h;
}
static size_t hh_snap_total(const HhSnapHeader &h) {
    size_t off = sizeof(HhSnapHeader);
    for (int i = 0; i < h.n_sections; i++) off = align_up(off, 16) + (size_t)h.section_bytes[i];
    return align_up(off, 16);
}
static void hh_snap_fill(HhSnapHeader &h, uint32_t magic, const HhSnapSection *s, int n) {
    h.magic = magic; h.version = HH_SNAP_VERSION; h.n_sections = n;
    for (int i = 0; i < HH_SNAP_MAX_SECTIONS; i++) h.section_bytes[i] = i < n ? s[i].bytes : 0;
}

/* device (and host) sections -> blob */
static int hh_snap_write(const HhSnapHeader &h, const HhSnapSection *s, void *buf, int64_t bytes, hipStream_t st, const char *who) {
    if (!buf || bytes < (int64_t)hh_snap_total(h)) { g_err = std::string(who) + ": the buffer is smaller than the snapshot (ask *_snapshot_bytes)"; return HH_E_ARG; }
    char *b = static_cast<char *>(buf);
    memset(b, 0, hh_snap_total(h)); /* the padding between sections is part of the blob: the same state gives the same bytes */
    memcpy(b, &h, sizeof(h));
    size_t off = sizeof(HhSnapHeader);
    for (int i = 0; i < h.n_sections; i++) {
        off = align_up(off, 16);
        if (s[i].bytes && s[i].dev) HIPCHK(hipMemcpyAsync(b + off, s[i].dev, s[i].bytes, hipMemcpyDeviceToHost, st));
        else if (s[i].bytes && s[i].host) memcpy(b + off, s[i].host, s[i].bytes);
        off += s[i].bytes;
    }
    HIPCHK(hipStreamSynchronize(st));
    return HH_OK;
}

/* the whole header against what the receiving object would write itself; nothing is written */
static int hh_snap_check(const HhSnapHeader &want, const void *buf, int64_t bytes, const char *who, const char *digest_what) {
    const std::string w(who);
    if (!buf || bytes < (int64_t)sizeof(HhSnapHeader)) { g_err = w + ": the buffer is shorter than a snapshot header"; return HH_E_ARG; }
    HhSnapHeader got;
    memcpy(&got, buf, sizeof(got));
    if (got.magic != want.magic) { g_err = w + ": not a snapshot of this kind of object (magic)"; return HH_E_ARG; }
    if (got.version != want.version) { g_err = w + ": snapshot format version " + std::to_string(got.version) + ", this library reads version " + std::to_string(want.version); return HH_E_ARG; }
    if (got.N != want.N || got.A != want.A || got.slots != want.slots) {
        g_err = w + ": the snapshot has N / A / slots = " + std::to_string(got.N) + " / " + std::to_string(got.A) + " / " + std::to_string(got.slots) + ", the receiving object " +
                std::to_string(want.N) + " / " + std::to_string(want.A) + " / " + std::to_string(want.slots);
        return HH_E_ARG;
    }
    if (got.digest != want.digest) { g_err = w + ": " + digest_what; return HH_E_ARG; }
    for (int i = 0; i < HH_SNAP_AUX; i++)
        if (got.aux[i] != want.aux[i]) { g_err = w + ": layout word " + std::to_string(i) + " differs (snapshot " + std::to_string(got.aux[i]) + ", receiving object " + std::to_string(want.aux[i]) + ")"; return HH_E_ARG; }
    if (got.n_sections != want.n_sections) { g_err = w + ": the snapshot has another number of sections"; return HH_E_ARG; }
    for (int i = 0; i < HH_SNAP_MAX_SECTIONS; i++)
        if (got.section_bytes[i] != want.section_bytes[i]) { g_err = w + ": section " + std::to_string(i) + " has another size than the receiving object's"; return HH_E_ARG; }
    if (bytes < (int64_t)hh_snap_total(want)) { g_err = w + ": the buffer is shorter than the snapshot its header describes (truncated)"; return HH_E_ARG; }
    return HH_OK;
}

/* blob -> the device sections (host sections are the caller's: they were compared, not copied) */
static int hh_snap_read(const HhSnapHeader &h, const HhSnapSection *s, const void *buf, hipStream_t st) {
    const char *b = static_cast<const char *>(buf);
    size_t off = sizeof(HhSnapHeader);
    for (int i = 0; i < h.n_sections; i++) {
        off = align_up(off, 16);
        if (s[i].bytes && s[i].dev) HIPCHK(hipMemcpyAsync(s[i].dev, b + off, s[i].bytes, hipMemcpyHostToDevice, st));
        off += s[i].bytes;
    }
    HIPCHK(hipStreamSynchronize(st));
    return HH_OK;
}

/* ---- world ---- */
static int hh_world_snap_layout(hh_world *w, HhSnapHeader &h, HhSnapSection *s) {
    memset(&h, 0, sizeof(h));
    const hh_policy *bank = w->bound_policy;
    s[0] = {nullptr, sizeof(hh_config), &w->cfg};
    s[1] = {w->slab, w->slab_bytes, nullptr};
    s[2] = {bank ? bank->counts : nullptr, bank ? HHP_COUNTS_INTS * sizeof(int) : 0, nullptr};
    s[3] = {bank ? bank->lists : nullptr, bank ? (size_t)HH_POLICY_MAX_NETS * bank->max_rows * sizeof(int) : 0, nullptr};
    hh_snap_fill(h, HH_SNAP_MAGIC_WORLD, s, 4);
    h.digest = hh_snap_fnv(&w->cfg, sizeof(hh_config));
    h.N = w->dc.N; h.A = w->dc.A; h.slots = 0;
    h.aux[0] = bank ? bank->max_rows : 0;
    return 4;
}

extern "C" int hh_world_snapshot_bytes(hh_world *w, int64_t *bytes) {
    if (!w || !bytes) { g_err = "hh_world_snapshot_bytes: null argument"; return HH_E_ARG; }
    HhSnapHeader h; HhSnapSection s[HH_SNAP_MAX_SECTIONS];
    hh_world_snap_layout(w, h, s);
    *bytes = (int64_t)hh_snap_total(h);
    return HH_OK;
}

extern "C" int hh_world_snapshot(hh_world *w, void *host_buf, int64_t bytes, void *stream) {
    if (!w) { g_err = "hh_world_snapshot: null argument"; return HH_E_ARG; }
    HhSnapHeader h; HhSnapSection s[HH_SNAP_MAX_SECTIONS];
    hh_world_snap_layout(w, h, s);
    HH_GUARD(w);
    return hh_snap_write(h, s, host_buf, bytes, (hipStream_t)stream, "hh_world_snapshot");
}

extern "C" int hh_world_restore(hh_world *w, const void *host_buf, int64_t bytes, void *stream) {
    if (!w) { g_err = "hh_world_restore: null argument"; return HH_E_ARG; }
    HhSnapHeader h; HhSnapSection s[HH_SNAP_MAX_SECTIONS];
    hh_world_snap_layout(w, h, s);
    /* the configuration first, field by field: the message names what differs (the digest alone could not) */
    if (host_buf && bytes >= (int64_t)(sizeof(HhSnapHeader) + sizeof(hh_config))) {
        HhSnapHeader got; hh_config c;
        memcpy(&got, host_buf, sizeof(got));
        memcpy(&c, static_cast<const char *>(host_buf) + sizeof(HhSnapHeader), sizeof(c));
        if (got.magic == h.magic && got.version == h.version && got.section_bytes[0] == sizeof(hh_config)) {
            const hh_config &m = w->cfg;
            const char *what = nullptr;
            if (c.n_arenas != m.n_arenas) what = "n_arenas";
            else if (c.env_kind != m.env_kind) what = "env_kind";
            else if (c.n_agents != m.n_agents || c.n_opps != m.n_opps) what = "n_agents / n_opps";
            else if (c.level != m.level) what = "level";
            else if (c.agent_mode != m.agent_mode) what = "agent_mode";
            else if (c.seed != m.seed) what = "seed";
            else if (c.arena_offset != m.arena_offset) what = "arena_offset";
            else if (c.horizon != m.horizon) what = "horizon";
            else if (c.ext_opp_actions != m.ext_opp_actions) what = "ext_opp_actions";
            else if (c.auto_reset != m.auto_reset) what = "auto_reset";
            if (what) { g_err = std::string("hh_world_restore: the snapshot's world was created with another ") + what; return HH_E_ARG; }
        }
    }
    int rc = hh_snap_check(h, host_buf, bytes, "hh_world_restore", "the snapshot's world was created with another hh_config (digest)");
    if (rc) return rc;
    if (memcmp(static_cast<const char *>(host_buf) + sizeof(HhSnapHeader), &w->cfg, sizeof(hh_config)) != 0) {
        g_err = "hh_world_restore: the snapshot's world was created with another hh_config"; return HH_E_ARG;
    }
    HH_GUARD(w);
    return hh_snap_read(h, s, host_buf, (hipStream_t)stream);
}

/* ---- policy bank ---- */
static int hh_policy_snap_layout(hh_policy *p, HhSnapHeader &h, HhSnapSection *s) {
    memset(&h, 0, sizeof(h));
    s[0] = {p->lut, 256, nullptr};
    s[1] = {p->counts, HHP_COUNTS_INTS * sizeof(int), nullptr};
    s[2] = {p->lists, (size_t)HH_POLICY_MAX_NETS * p->max_rows * sizeof(int), nullptr};
    h.aux[0] = p->binned_rows;
    return 3;
}
/* slot `slot`'s parts in HH_POLICY_PART_* order: device range k of n (a slot is one section of several ranges) */
static int hh_policy_slot_parts(hh_policy *p, int slot, const char *src[5], int64_t n[5]) {
    int k = 0;
    if (!p->blob[slot]) return 0;
    const bool crit = p->cbank.c[slot].loaded && p->cbankx.c[slot].loaded;
    for (int part = 0; part < (crit ? 5 : 3); part++) {
        if (hhr_policy_part(p, slot, part, &src[k], &n[k]) != HH_OK) return -1;
        k++;
    }
    return k;
}

static int hh_policy_snap_run(hh_policy *p, void *wbuf, const void *rbuf, int64_t bytes, int64_t *size_only, hipStream_t st, const char *who) {
    HhSnapHeader h; HhSnapSection s[HH_SNAP_MAX_SECTIONS];
    hh_policy_snap_layout(p, h, s);
    const char *src[HH_POLICY_MAX_NETS][5];
    int64_t n[HH_POLICY_MAX_NETS][5];
    int parts[HH_POLICY_MAX_NETS];
    for (int slot = 0; slot < HH_POLICY_MAX_NETS; slot++) {
        parts[slot] = hh_policy_slot_parts(p, slot, src[slot], n[slot]);
        if (parts[slot] < 0) return HH_E_ARG;
        size_t tot = 0;
        for (int k = 0; k < parts[slot]; k++) tot += align_up((size_t)n[slot][k], 16);
        s[3 + slot] = {nullptr, tot, nullptr}; /* copied range by range below */
        h.aux[1 + slot] = parts[slot] == 0 ? -1 : (p->bank.net[slot].kind | (parts[slot] == 5 ? 16 : 0));
    }
    hh_snap_fill(h, HH_SNAP_MAGIC_POLICY, s, 3 + HH_POLICY_MAX_NETS);
    h.N = p->max_rows; h.A = 0; h.slots = HH_POLICY_MAX_NETS;
    /* the geometry: what the slots hold and how large every packed part is */
    h.digest = hh_snap_fnv(&h.aux[1], HH_POLICY_MAX_NETS * sizeof(int32_t));
    for (int slot = 0; slot < HH_POLICY_MAX_NETS; slot++) h.digest = hh_snap_fnv(n[slot], (size_t)parts[slot] * sizeof(int64_t), h.digest);
    if (size_only) { *size_only = (int64_t)hh_snap_total(h); return HH_OK; }
    if (rbuf) {
        /* binned_rows is state, not layout: taken from the blob after the check */
        if (bytes >= (int64_t)sizeof(HhSnapHeader)) { HhSnapHeader got; memcpy(&got, rbuf, sizeof(got)); h.aux[0] = got.aux[0]; }
        int rc = hh_snap_check(h, rbuf, bytes, who, "the snapshot's bank holds other networks than the receiving bank (slot layout digest)");
        if (rc) return rc;
    }
    DeviceGuard guard_(p->device);
    if (!guard_.ok) { g_err = "hipSetDevice(bank device) failed"; return HH_E_HIP; }
    if (wbuf) { int rc = hh_snap_write(h, s, wbuf, bytes, st, who); if (rc) return rc; }
    else { int rc = hh_snap_read(h, s, rbuf, st); if (rc) return rc; }
    size_t off = sizeof(HhSnapHeader);
    for (int i = 0; i < 3 + HH_POLICY_MAX_NETS; i++) {
        off = align_up(off, 16);
        if (i >= 3) {
            size_t o = off;
            for (int k = 0; k < parts[i - 3]; k++) {
                if (wbuf) HIPCHK(hipMemcpyAsync(static_cast<char *>(wbuf) + o, src[i - 3][k], (size_t)n[i - 3][k], hipMemcpyDeviceToHost, st));
                else HIPCHK(hipMemcpyAsync(const_cast<char *>(src[i - 3][k]), static_cast<const char *>(rbuf) + o, (size_t)n[i - 3][k], hipMemcpyHostToDevice, st));
                o += align_up((size_t)n[i - 3][k], 16);
            }
        }
        off += (size_t)h.section_bytes[i];
    }
    HIPCHK(hipStreamSynchronize(st));
    if (rbuf) p->binned_rows = h.aux[0];
    return HH_OK;
}

extern "C" int hh_policy_snapshot_bytes(hh_policy *p, int64_t *bytes) {
    if (!p || !bytes) { g_err = "hh_policy_snapshot_bytes: null argument"; return HH_E_ARG; }
    return hh_policy_snap_run(p, nullptr, nullptr, 0, bytes, nullptr, "hh_policy_snapshot_bytes");
}
extern "C" int hh_policy_snapshot(hh_policy *p, void *host_buf, int64_t bytes, void *stream) {
    if (!p || !host_buf) { g_err = "hh_policy_snapshot: null argument"; return HH_E_ARG; }
    return hh_policy_snap_run(p, host_buf, nullptr, bytes, nullptr, (hipStream_t)stream, "hh_policy_snapshot");
}
extern "C" int hh_policy_restore(hh_policy *p, const void *host_buf, int64_t bytes, void *stream) {
    if (!p || !host_buf) { g_err = "hh_policy_restore: null argument"; return HH_E_ARG; }
    return hh_policy_snap_run(p, nullptr, host_buf, bytes, nullptr, (hipStream_t)stream, "hh_policy_restore");
}

/* ---- commander ---- */
static void hh_commander_snap_layout(hh_commander *c, HhSnapHeader &h, HhSnapSection *s) {
    memset(&h, 0, sizeof(h));
    const bool on = c->loaded && c->blob;
    s[0] = {on ? c->blob : nullptr, on ? (size_t)(reinterpret_cast<const char *>(c->net.br[1].bo + 4) - c->blob) : 0, nullptr};
    hh_snap_fill(h, HH_SNAP_MAGIC_COMMANDER, s, 1);
    h.N = 0; h.A = HH_CMD_AGENTS; h.slots = 1;
    h.aux[0] = on ? 1 : 0;
    const int32_t geo[5] = {HH_CMD_OBS, HH_CMD_AGENTS, HH_CMD_HIDDEN, HH_CMD_ACTIONS, (int32_t)s[0].bytes};
    h.digest = hh_snap_fnv(geo, sizeof(geo));
}
extern "C" int hh_commander_snapshot_bytes(hh_commander *c, int64_t *bytes) {
    if (!c || !bytes) { g_err = "hh_commander_snapshot_bytes: null argument"; return HH_E_ARG; }
    HhSnapHeader h; HhSnapSection s[HH_SNAP_MAX_SECTIONS];
    hh_commander_snap_layout(c, h, s);
    *bytes = (int64_t)hh_snap_total(h);
    return HH_OK;
}
extern "C" int hh_commander_snapshot(hh_commander *c, void *host_buf, int64_t bytes, void *stream) {
    if (!c) { g_err = "hh_commander_snapshot: null argument"; return HH_E_ARG; }
    HhSnapHeader h; HhSnapSection s[HH_SNAP_MAX_SECTIONS];
    hh_commander_snap_layout(c, h, s);
    HH_GUARD(c);
    return hh_snap_write(h, s, host_buf, bytes, (hipStream_t)stream, "hh_commander_snapshot");
}
extern "C" int hh_commander_restore(hh_commander *c, const void *host_buf, int64_t bytes, void *stream) {
    if (!c) { g_err = "hh_commander_restore: null argument"; return HH_E_ARG; }
    HhSnapHeader h; HhSnapSection s[HH_SNAP_MAX_SECTIONS];
    hh_commander_snap_layout(c, h, s);
    int rc = hh_snap_check(h, host_buf, bytes, "hh_commander_restore", "the snapshot's commander has another geometry (digest)");
    if (rc) return rc;
    HH_GUARD(c);
    return hh_snap_read(h, s, host_buf, (hipStream_t)stream);
}

#endif /* HH_SNAPSHOT_H */
