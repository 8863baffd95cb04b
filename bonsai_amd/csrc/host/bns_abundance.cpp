// bns_abundance.cpp -- `bonsai abundance`: the reads of a `classify -R` report re-estimated at one taxonomic level with the window
// distribution `bonsai distrib` wrote for the same db, read length and confidence threshold.  Host code only: no device is involved.
// The project's own definition (DESIGN "Defined behaviour"), after Bracken's re-estimation as recalled and not checked against Bracken.
#include "bns_host_internal.hpp"

#include <sstream>

namespace bns {
namespace {

constexpr u32 NOT_IN_TAXONOMY = 0xFFFFFFFFu;         // the taxid `classify -R` prints on its "(not in taxonomy)" line

std::vector<std::string_view> split(std::string_view s, char sep)
{
    std::vector<std::string_view> f;
    size_t at = 0;
    for (;;) {
        const size_t e = s.find(sep, at);
        f.push_back(s.substr(at, e == std::string_view::npos ? std::string_view::npos : e - at));
        if (e == std::string_view::npos) break;
        at = e + 1;
    }
    return f;
}

// digits only, a value that fits 64 bits
bool parse_u64(std::string_view s, u64 &out)
{
    if (s.empty() || s.size() > 20) return false;
    u64 v = 0;
    for (char ch : s) {
        if (ch < '0' || ch > '9') return false;
        const u64 d = (u64)(ch - '0');
        if (v > (~0ULL - d) / 10) return false;
        v = v * 10 + d;
    }
    out = v;
    return true;
}

std::vector<std::string_view> lines_of(const std::string &text)
{
    std::vector<std::string_view> l = split(text, '\n');
    if (!l.empty() && l.back().empty()) l.pop_back();            // (the text ends with a line end)
    return l;
}

struct DistribEntry { u32 genome; u64 here, all; };

std::map<u32, std::vector<DistribEntry>> parse_distrib(const std::string &text)
{
    const std::vector<std::string_view> lines = lines_of(text);
    auto bad = [](size_t i, const char *why) { die("distrib file, line " + std::to_string(i + 1) + ": " + why); };
    if (lines.empty() || lines[0] != "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers") bad(0, "not the header `bonsai distrib` writes");
    std::map<u32, std::vector<DistribEntry>> out;
    for (size_t i = 1; i < lines.size(); ++i) {
        const auto f = split(lines[i], '\t');
        u64 t = 0;
        if (f.size() != 2 || !parse_u64(f[0], t) || t == 0 || t >= NOT_IN_TAXONOMY) bad(i, "expected <taxid><TAB><entries>");
        if (out.count((u32)t)) bad(i, "a second line for this taxid");
        std::vector<DistribEntry> &v = out[(u32)t];
        for (std::string_view e : split(f[1], ' ')) {
            const auto p = split(e, ':');
            u64 g = 0, w = 0, W = 0;
            if (p.size() != 3 || !parse_u64(p[0], g) || !parse_u64(p[1], w) || !parse_u64(p[2], W) || g > NOT_IN_TAXONOMY)
                bad(i, "an entry is <genome taxid>:<windows called here>:<all windows of the genome>");
            if (W == 0 || w > W) bad(i, "an entry's windows called here exceed all windows of the genome, or there are none");
            v.push_back({(u32)g, w, W});
        }
        std::stable_sort(v.begin(), v.end(), [](const DistribEntry &a, const DistribEntry &b) { return a.genome < b.genome; });
    }
    return out;
}

// taxid -> direct count of every line of a `classify -R` report (6, 7 or 9 fields; read from the right)
std::map<u32, u64> parse_report(const std::string &text)
{
    const std::vector<std::string_view> lines = lines_of(text);
    auto bad = [](size_t i, const char *why) { die("report file, line " + std::to_string(i + 1) + ": " + why); };
    std::map<u32, u64> direct;
    for (size_t i = 0; i < lines.size(); ++i) {
        const auto f = split(lines[i], '\t');
        const size_t n = f.size();
        if (n != 6 && n != 7 && n != 9) bad(i, "a report line has 6, 7 or 9 tab-separated fields");
        u64 taxid = 0, d = 0;
        if (!parse_u64(f[n - 2], taxid) || taxid > NOT_IN_TAXONOMY) bad(i, "the taxid (the field before the name) is no number below 2^32");
        if (!parse_u64(f[2], d)) bad(i, "the direct count (the third field) is no number");
        if (f[n - 3].empty()) bad(i, "the rank code is empty");
        if (!direct.emplace((u32)taxid, d).second) bad(i, "a second line for this taxid");
    }
    return direct;
}

}  // namespace

std::string estimate_abundance(const std::string &distrib_text, const std::string &report_text, const std::vector<u32> &parent,
                               const std::vector<std::string> &ranks, const std::unordered_map<u32, std::string> &names,
                               const AbundanceOptions &opt, double totals[5])
{
    const std::string letter(1, opt.level);
    if (std::string("DKPCOFGS").find(opt.level) == std::string::npos || opt.level == '\0') die("-l: the level is one of D K P C O F G S");
    const std::map<u32, std::vector<DistribEntry>> distrib = parse_distrib(distrib_text);
    const std::map<u32, u64> direct = parse_report(report_text);
    const u32 n = (u32)parent.size();
    // the first of t, parent(t), ... whose own rank maps to the level's letter; 0: none
    auto level_of = [&](u32 t) -> u32 {
        for (u32 steps = 0; t != 0 && t < n && steps <= n; ++steps) {
            if (t < ranks.size() && letter == rank_letter(ranks[t])) return t;
            const u32 p = parent[t];
            if (p == BNS_TAX_ABSENT || p == t) break;
            t = p;
        }
        return 0;
    };
    u64 all = 0, unclassified = 0, discarded = 0, not_distributed = 0;
    std::map<u32, u64> base;                                     // level node -> the reads at it and below it
    std::vector<std::pair<u32, u64>> above;                      // taxa with reads and no level node on their chain
    for (const auto &kv : direct) {
        all += kv.second;
        if (kv.first == 0 || kv.first == NOT_IN_TAXONOMY) { unclassified += kv.second; continue; }
        if (!kv.second) continue;
        const u32 s = level_of(kv.first);
        if (s) base[s] += kv.second; else above.push_back(kv);
    }
    std::map<u32, double> added;                                 // the kept level nodes
    for (const auto &kv : base) {
        if (kv.second >= opt.min_reads) added[kv.first] = 0.0; else discarded += kv.second;
    }
    for (const auto &nv : above) {
        const auto line = distrib.find(nv.first);
        std::map<u32, double> weight;
        double sum = 0.0;
        if (line != distrib.end())
            for (const DistribEntry &e : line->second) {         // (genomes in ascending taxid)
                const u32 s = level_of(e.genome);
                if (!s || !added.count(s)) continue;
                const double w = (double)e.here / (double)e.all * (double)base[s];
                weight[s] += w;
                sum += w;
            }
        if (!(sum > 0.0)) { not_distributed += nv.second; continue; }
        for (const auto &w : weight) added[w.first] += (double)nv.second * w.second / sum;
    }
    double est_sum = 0.0;
    for (const auto &kv : added) est_sum += (double)base[kv.first] + kv.second;
    std::string out = "name\ttaxonomy_id\ttaxonomy_lvl\tkraken_assigned_reads\tadded_reads\tnew_est_reads\tfraction_total_reads\n";
    for (const auto &kv : added) {
        const auto nm = names.find(kv.first);
        const double est = (double)base[kv.first] + kv.second;
        char buf[160];
        std::snprintf(buf, sizeof(buf), "\t%u\t%c\t%llu\t%.3f\t%.3f\t%.6f\n", kv.first, opt.level, (unsigned long long)base[kv.first], kv.second, est,
                      est_sum > 0.0 ? est / est_sum : 0.0);
        out += nm != names.end() ? nm->second : std::to_string(kv.first);
        out += buf;
    }
    if (totals) {
        totals[0] = (double)all; totals[1] = (double)unclassified; totals[2] = (double)discarded; totals[3] = (double)not_distributed;
        totals[4] = est_sum;
    }
    return out;
}

std::string read_text_file(const char *path)
{
    std::ifstream is(path, std::ios::binary);
    if (!is) die(std::string("Could not open ") + path + " for reading.");
    std::ostringstream ss;
    ss << is.rdbuf();
    return ss.str();
}

std::string estimate_abundance_files(const char *distrib_path, const char *report_path, const char *nodes_dmp, const char *names_dmp,
                                     const AbundanceOptions &opt, double totals[5])
{
    const std::vector<u32> parent = build_parent_map(nodes_dmp);
    const std::vector<std::string> ranks = read_node_ranks(nodes_dmp);
    const std::unordered_map<u32, std::string> names = names_dmp ? read_scientific_names(names_dmp) : std::unordered_map<u32, std::string>{};
    return estimate_abundance(read_text_file(distrib_path), read_text_file(report_path), parent, ranks, names, opt, totals);
}

}  // namespace bns
