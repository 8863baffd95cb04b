// bns_report.cpp -- the per-sample taxon report of `bonsai classify -R` (Kraken 2's standard report layout): nodes.dmp ranks,
// names.dmp scientific names, the text, and the read-out of the device tallies.  The counting itself runs on the device
// (bns_tally_enable / bns_tally_read: tally_kernel, clade_kernel).  No reference counterpart: the reference counts classified and
// unclassified reads (classifier.h:138,238) and prints neither.  `-u` adds a column: the distinct k-mers of each node's clade, estimated
// from the device's HyperLogLog sketches (bns_sketch_enable / bns_sketch_read), merged up the taxonomy here.
#include "bns_host_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <map>

namespace bns {
namespace {

// the '|'-separated fields of a .dmp line, tabs and spaces around each trimmed
std::vector<std::string_view> dmp_fields(std::string_view line)
{
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.remove_suffix(1);
    std::vector<std::string_view> f;
    size_t at = 0;
    for (;;) {
        const size_t bar = line.find('|', at);
        std::string_view x = line.substr(at, bar == std::string_view::npos ? std::string_view::npos : bar - at);
        while (!x.empty() && (x.front() == '\t' || x.front() == ' ')) x.remove_prefix(1);
        while (!x.empty() && (x.back() == '\t' || x.back() == ' ')) x.remove_suffix(1);
        f.push_back(x);
        if (bar == std::string_view::npos) break;
        at = bar + 1;
    }
    return f;
}

}  // namespace

const char *rank_letter(const std::string &r)
{
    if (r == "superkingdom" || r == "domain") return "D";
    if (r == "kingdom") return "K";
    if (r == "phylum") return "P";
    if (r == "class") return "C";
    if (r == "order") return "O";
    if (r == "family") return "F";
    if (r == "genus") return "G";
    if (r == "species") return "S";
    return "";
}

namespace {

// distinct: the extra column of the `-u` report (nullptr: the seven-column line); db_keys: the two columns `-d` puts behind it, the
// clade's key count in the db and distinct / db_keys (not clamped: the numerator is an estimate), 0.000000 where the db holds none
void report_line(std::string &out, u64 clade, u64 direct, const u64 *distinct, const u64 *db_keys, u64 total, const std::string &code, u32 taxid,
                 unsigned depth, const std::string &name)
{
    char head[224];
    const double pct = total ? 100.0 * (double)clade / (double)total : 0.0;
    if (distinct && db_keys)
        std::snprintf(head, sizeof(head), "%6.2f\t%llu\t%llu\t%llu\t%llu\t%.6f\t%s\t%u\t", pct, (unsigned long long)clade, (unsigned long long)direct,
                      (unsigned long long)*distinct, (unsigned long long)*db_keys, *db_keys ? (double)*distinct / (double)*db_keys : 0.0,
                      code.c_str(), taxid);
    else if (distinct)
        std::snprintf(head, sizeof(head), "%6.2f\t%llu\t%llu\t%llu\t%s\t%u\t", pct, (unsigned long long)clade, (unsigned long long)direct,
                      (unsigned long long)*distinct, code.c_str(), taxid);
    else
        std::snprintf(head, sizeof(head), "%6.2f\t%llu\t%llu\t%s\t%u\t", pct, (unsigned long long)clade, (unsigned long long)direct, code.c_str(), taxid);
    out += head;
    out.append((size_t)depth * 2, ' ');
    out += name;
    out += '\n';
}

// distinct[v], v in [0, n]: the estimate of the register-wise maximum over the sketched bins in v's subtree (0: none there); bin n its own,
// bin 0 left at 0 (the unclassified line has no k-mers).  The nodes that matter are the sketched bins and their ancestors: each is
// visited once, children before parents (a node is ready when its last child with a sketch has been merged into it), and each sketch is
// merged into its parent's once -- no sketch walks its whole chain.
std::vector<u64> clade_distinct(const u32 *bins, const u8 *regs, u32 n_sk, u32 n, const u32 *parent)
{
    std::vector<u64> distinct((size_t)n + 1, 0);
    std::vector<u32> idx(n, 0xFFFFFFFFu);                  // node -> its entry in the three vectors below
    std::vector<u32> node, pending;
    std::vector<std::vector<u8>> sk;
    auto up = [&](u32 v) -> u32 { const u32 p = parent[v]; return (p == 0 || p >= n || p == v) ? 0u : p; };
    for (u32 i = 0; i < n_sk; ++i) {
        const u32 b = bins[i];
        const u8 *r = regs + (size_t)i * HLL_M;
        if (b == n) { distinct[n] = hll_estimate(r); continue; }
        if (b == 0 || b > n) continue;
        for (u32 v = b, prev = 0xFFFFFFFFu; v; v = up(v)) {            // b and its ancestors, up to the first one already known
            const bool known = idx[v] != 0xFFFFFFFFu;
            if (!known) { idx[v] = (u32)node.size(); node.push_back(v); pending.push_back(0); sk.emplace_back(); }
            if (prev != 0xFFFFFFFFu) ++pending[idx[v]];
            prev = v;
            if (known || node.size() > n) break;
        }
        sk[idx[b]].assign(r, r + HLL_M);
    }
    std::vector<u32> ready;
    for (u32 e = 0; e < node.size(); ++e) if (!pending[e]) ready.push_back(e);
    while (!ready.empty()) {
        const u32 e = ready.back();
        ready.pop_back();
        const u32 v = node[e], p = up(v);
        if (!sk[e].empty()) distinct[v] = hll_estimate(sk[e].data());
        if (p && idx[p] != 0xFFFFFFFFu) {
            std::vector<u8> &ps = sk[idx[p]];
            if (ps.empty()) ps.swap(sk[e]);
            else if (!sk[e].empty()) for (u32 j = 0; j < HLL_M; ++j) ps[j] = std::max(ps[j], sk[e][j]);
            if (--pending[idx[p]] == 0) ready.push_back(idx[p]);
        }
        std::vector<u8>().swap(sk[e]);                     // (merged: only the frontier's sketches are held)
    }
    return distinct;
}

}  // namespace

u64 hll_estimate(const u8 *reg)
{
    u32 cnt[64] = {0};
    for (u32 j = 0; j < HLL_M; ++j) ++cnt[reg[j] & 63u];
    if (cnt[0] == HLL_M) return 0;
    const double m = (double)HLL_M;
    double sum = 0.0;                                      // sum of 2^-reg[j], rank by rank in ascending order (a fixed order: reproducible)
    for (int r = 0; r < 64; ++r) sum += (double)cnt[r] * std::ldexp(1.0, -r);
    double e = 0.7213 / (1.0 + 1.079 / m) * m * m / sum;
    if (e <= 2.5 * m && cnt[0]) e = m * std::log(m / (double)cnt[0]);
    return e < 18446744073709549568.0 ? (u64)std::floor(e + 0.5) : ~0ULL;      // (every register near 53: past what a u64 holds)
}

std::vector<std::string> read_node_ranks(const char *nodes_dmp)
{
    std::ifstream is(nodes_dmp);
    if (!is) die(std::string("Could not open ") + nodes_dmp + " for reading.");
    std::vector<std::string> rank;
    std::string line;
    while (std::getline(is, line)) {
        if (line.empty() || line[0] == '#') continue;                       // (as build_parent_map skips them)
        const auto f = dmp_fields(line);
        const u32 id = (u32)std::atoi(line.c_str());
        if (id >= (1u << 28)) die("taxid >= 2^28 is not supported by the flat parent array");
        if (id >= rank.size()) rank.resize((size_t)id + 1);
        rank[id] = f.size() >= 3 && !f[2].empty() ? std::string(f[2]) : std::string("no rank");   // (later lines win, as for the parent)
    }
    return rank;
}

std::unordered_map<u32, std::string> read_scientific_names(const char *names_dmp)
{
    std::ifstream is(names_dmp);
    if (!is) die(std::string("Could not open ") + names_dmp + " for reading.");
    std::unordered_map<u32, std::string> names;
    std::string line;
    while (std::getline(is, line)) {
        if (line.empty() || line[0] == '#') continue;
        const auto f = dmp_fields(line);
        if (f.size() < 4 || f[3] != "scientific name") continue;
        names.emplace((u32)std::atoi(line.c_str()), std::string(f[1]));      // (the first one of a taxid stays)
    }
    return names;
}

namespace {
std::string format_report_impl(const u64 *direct, const u64 *clade, u32 n, const u32 *parent, const std::vector<std::string> &ranks,
                               const std::unordered_map<u32, std::string> &names, const u64 *distinct, const u64 *db_keys)
{
    if (!distinct) db_keys = nullptr;                      // (the coverage columns follow the distinct k-mer column)
    const u64 zero = 0;
    u64 total = 0;
    for (u32 v = 0; v <= n; ++v) total += direct[v];
    std::string out;
    if (direct[0]) report_line(out, direct[0], direct[0], distinct ? &zero : nullptr, db_keys ? &zero : nullptr, total, "U", 0u, 0u, "unclassified");
    // children lists of the nodes with a count, in print order: clade descending, ties by taxid ascending
    std::vector<u32> child_cnt(n + 1, 0);
    std::vector<u32> roots;
    for (u32 v = 1; v < n; ++v) {
        if (!clade[v]) continue;
        const u32 p = parent[v];
        if (p == 0) roots.push_back(v);
        else if (p < n && p != v) ++child_cnt[p];
    }
    std::vector<u32> off(n + 1, 0);
    for (u32 v = 0; v < n; ++v) off[v + 1] = off[v] + child_cnt[v];
    std::vector<u32> kids(off[n]);
    {
        std::vector<u32> fill(off.begin(), off.end() - 1);
        for (u32 v = 1; v < n; ++v) if (clade[v] && parent[v] != 0 && parent[v] < n && parent[v] != v) kids[fill[parent[v]]++] = v;
    }
    for (u32 v = 1; v < n; ++v)
        std::sort(kids.begin() + off[v], kids.begin() + off[v + 1], [&](u32 a, u32 b) { return clade[a] != clade[b] ? clade[a] > clade[b] : a < b; });
    auto name_of = [&](u32 v) { const auto it = names.find(v); return it != names.end() ? it->second : std::to_string(v); };
    auto letter_of = [&](u32 v) -> std::string {
        if (v == 1) return "R";
        return v < ranks.size() ? rank_letter(ranks[v]) : "";
    };
    // depth-first from each root (an explicit stack: a chain may be deep); a rank without a letter takes the nearest lettered
    // ancestor's, followed by the number of steps from it ("-" when no ancestor has one)
    struct Frame { u32 v, depth, steps; std::string base; };
    for (u32 r : roots) {
        std::vector<Frame> st;
        st.push_back({r, 0u, 0u, ""});
        while (!st.empty()) {
            Frame f = std::move(st.back());
            st.pop_back();
            const std::string own = letter_of(f.v);
            if (!own.empty()) { f.base = own; f.steps = 0; }
            else if (!f.base.empty()) ++f.steps;
            const std::string code = f.base.empty() ? std::string("-") : f.steps ? f.base + std::to_string(f.steps) : f.base;
            report_line(out, clade[f.v], direct[f.v], distinct ? distinct + f.v : nullptr, db_keys ? db_keys + f.v : nullptr, total, code, f.v, f.depth, name_of(f.v));
            for (u32 i = off[f.v + 1]; i-- > off[f.v];) st.push_back({kids[i], f.depth + 1, f.steps, f.base});   // (first child on top)
        }
    }
    if (direct[n]) report_line(out, direct[n], direct[n], distinct ? distinct + n : nullptr, db_keys ? db_keys + n : nullptr, total, "-", 0xFFFFFFFFu, 0u, "(not in taxonomy)");
    return out;
}
}  // namespace

std::string format_report(const u64 *direct, const u64 *clade, u32 n, const u32 *parent, const std::vector<std::string> &ranks,
                          const std::unordered_map<u32, std::string> &names)
{
    return format_report_impl(direct, clade, n, parent, ranks, names, nullptr, nullptr);
}

std::string format_report(const u64 *direct, const u64 *clade, u32 n, const u32 *parent, const std::vector<std::string> &ranks,
                          const std::unordered_map<u32, std::string> &names, const u32 *sketch_bins, const u8 *sketch_regs, u32 n_sketched,
                          const u64 *db_keys)
{
    const std::vector<u64> distinct = clade_distinct(sketch_bins, sketch_regs, n_sketched, n, parent);
    return format_report_impl(direct, clade, n, parent, ranks, names, distinct.data(), db_keys);
}

void enable_tally(ClassifierGeneric &c)
{
    for (bns_ctx *cx : c.ctxs_) chk(cx, bns_tally_enable(cx, 1), "bns_tally_enable");
}

void enable_sketch(ClassifierGeneric &c, u32 max_taxa)
{
    for (bns_ctx *cx : c.ctxs_) chk(cx, bns_sketch_enable(cx, max_taxa), "bns_sketch_enable");
    c.sketch_on_ = true;
}

void write_inspect(ClassifierGeneric &c, const Database &db, const std::vector<u32> &parent, const char *nodes_dmp, const char *names_dmp, std::FILE *out)
{
    const u32 n = (u32)parent.size();
    bns_ctx *cx = c.ctxs_[0];
    std::vector<u64> direct((size_t)n + 1, 0), clade((size_t)n + 1, 0);
    chk(cx, bns_table_tally(cx, direct.data(), clade.data(), n + 1), "bns_table_tally");
    uint64_t n_keys = 0, bytes = 0, geo[8] = {0};
    int layout = -1;
    chk(cx, bns_table_info(cx, &n_keys, &bytes, &layout), "bns_table_info");
    chk(cx, bns_table_geometry(cx, geo), "bns_table_geometry");
    const char *lname = layout == BNS_LAYOUT_KHASH ? "khash" : layout == BNS_LAYOUT_BUCKET ? "bucket" : "minbucket";
    const std::vector<std::string> ranks = read_node_ranks(nodes_dmp);
    const std::unordered_map<u32, std::string> names = names_dmp ? read_scientific_names(names_dmp) : std::unordered_map<u32, std::string>{};
    const std::string text = format_report(direct.data(), clade.data(), n, parent.data(), ranks, names);
    if (std::fprintf(out, "# k\t%u\n# keys\t%llu\n# layout\t%s\n# buckets\t%llu\n# window\t%llu\n# overflow keys\t%llu\n", db.k_, (unsigned long long)n_keys,
                     lname, (unsigned long long)geo[0], (unsigned long long)geo[4], (unsigned long long)geo[5]) < 0 ||
        std::fwrite(text.data(), 1, text.size(), out) != text.size())
        die("Could not write the inspect report");
}

void write_report(ClassifierGeneric &c, const std::vector<u32> &parent, const char *nodes_dmp, const char *names_dmp)
{
    const u32 n = (u32)parent.size();
    std::vector<u64> direct(n + 1, 0), clade(n + 1, 0), d(n + 1), cl(n + 1);
    for (bns_ctx *cx : c.ctxs_) {                                           // one tally per context; sums of both kinds add up
        chk(cx, bns_tally_read(cx, d.data(), cl.data(), n + 1, 0), "bns_tally_read");
        for (u32 v = 0; v <= n; ++v) { direct[v] += d[v]; clade[v] += cl[v]; }
    }
    const std::vector<std::string> ranks = read_node_ranks(nodes_dmp);
    const std::unordered_map<u32, std::string> names = names_dmp ? read_scientific_names(names_dmp) : std::unordered_map<u32, std::string>{};
    std::string text;
    if (c.sketch_on_) {
        // one set of sketches per context: equal bins merge by the register-wise maximum (bins come back ascending)
        std::map<u32, std::vector<u8>> merged;
        u64 dropped = 0;
        for (bns_ctx *cx : c.ctxs_) {
            u32 s = 0, dr = 0;
            chk(cx, bns_sketch_read(cx, nullptr, nullptr, 0, &s, &dr, 0), "bns_sketch_read");
            std::vector<u32> bins(s);
            std::vector<u8> regs((size_t)s * HLL_M);
            chk(cx, bns_sketch_read(cx, bins.data(), regs.data(), s, &s, &dr, 0), "bns_sketch_read");
            dropped += dr;
            for (u32 i = 0; i < s; ++i) {
                const u8 *r = regs.data() + (size_t)i * HLL_M;
                std::vector<u8> &m = merged[bins[i]];
                if (m.empty()) m.assign(r, r + HLL_M);
                else for (u32 j = 0; j < HLL_M; ++j) m[j] = std::max(m[j], r[j]);
            }
        }
        if (dropped)
            std::fprintf(stderr, "[W] -u: %llu taxon bins got no sketch (-U sets how many there are): the distinct k-mer column is a lower bound for their clades\n",
                         (unsigned long long)dropped);
        std::vector<u32> bins;
        std::vector<u8> regs;
        bins.reserve(merged.size()); regs.reserve(merged.size() * HLL_M);
        for (const auto &kv : merged) { bins.push_back(kv.first); regs.insert(regs.end(), kv.second.begin(), kv.second.end()); }
        // -d: the clades' key counts in the db.  Every context holds the same table: context 0's walk is the whole answer
        std::vector<u64> db_keys;
        if (c.coverage_on_) {
            db_keys.resize((size_t)n + 1);
            chk(c.ctxs_[0], bns_table_tally(c.ctxs_[0], nullptr, db_keys.data(), n + 1), "bns_table_tally");
        }
        text = format_report(direct.data(), clade.data(), n, parent.data(), ranks, names, bins.data(), regs.data(), (u32)bins.size(),
                             c.coverage_on_ ? db_keys.data() : nullptr);
    } else text = format_report(direct.data(), clade.data(), n, parent.data(), ranks, names);
    if (!c.report_out_ || std::fwrite(text.data(), 1, text.size(), c.report_out_) != text.size()) die("Could not write the report");
}

}  // namespace bns
