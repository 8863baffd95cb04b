// bns_report.cpp -- the per-sample taxon report of `bonsai classify -R` (Kraken 2's standard report layout): nodes.dmp ranks,
// names.dmp scientific names, the text, and the read-out of the device tallies.  The counting itself runs on the device
// (bns_tally_enable / bns_tally_read: tally_kernel, clade_kernel).  No reference counterpart: the reference counts classified and
// unclassified reads (classifier.h:138,238) and prints neither.
#include "bns_host_internal.hpp"

#include <algorithm>
#include <cstring>
#include <fstream>

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

// Kraken 2's rank letters; "" for a rank without one
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

void report_line(std::string &out, u64 clade, u64 direct, u64 total, const std::string &code, u32 taxid, unsigned depth, const std::string &name)
{
    char head[128];
    const double pct = total ? 100.0 * (double)clade / (double)total : 0.0;
    std::snprintf(head, sizeof(head), "%6.2f\t%llu\t%llu\t%s\t%u\t", pct, (unsigned long long)clade, (unsigned long long)direct, code.c_str(), taxid);
    out += head;
    out.append((size_t)depth * 2, ' ');
    out += name;
    out += '\n';
}

}  // namespace

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

std::string format_report(const u64 *direct, const u64 *clade, u32 n, const u32 *parent, const std::vector<std::string> &ranks,
                          const std::unordered_map<u32, std::string> &names)
{
    u64 total = 0;
    for (u32 v = 0; v <= n; ++v) total += direct[v];
    std::string out;
    if (direct[0]) report_line(out, direct[0], direct[0], total, "U", 0u, 0u, "unclassified");
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
            report_line(out, clade[f.v], direct[f.v], total, code, f.v, f.depth, name_of(f.v));
            for (u32 i = off[f.v + 1]; i-- > off[f.v];) st.push_back({kids[i], f.depth + 1, f.steps, f.base});   // (first child on top)
        }
    }
    if (direct[n]) report_line(out, direct[n], direct[n], total, "-", 0xFFFFFFFFu, 0u, "(not in taxonomy)");
    return out;
}

void enable_tally(ClassifierGeneric &c)
{
    for (bns_ctx *cx : c.ctxs_) chk(cx, bns_tally_enable(cx, 1), "bns_tally_enable");
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
    const std::string text = format_report(direct.data(), clade.data(), n, parent.data(), ranks, names);
    if (!c.report_out_ || std::fwrite(text.data(), 1, text.size(), c.report_out_) != text.size()) die("Could not write the report");
}

}  // namespace bns
