// tool_common_check.cpp — the device-free parts of genome_amd/host/tool_common.hpp (the argv cursor, the option groups, the JSON
// renderers), run as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer.  It links no library: nothing
// here touches the classes of genome.hpp, so none of their inline code is emitted.  tests/test_host_cli_cpu.py builds and runs it.
#include <cstdio>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../genome_amd/host/tool_common.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

// an argv of exactly these tokens (no terminating null, no slack: reading past the end is an error the sanitizer sees)
struct Argv {
    std::vector<std::string> words;
    std::vector<char *> ptrs;
    Argv(std::initializer_list<const char *> w) : words(w.begin(), w.end()) {
        for (auto &s : words) ptrs.push_back(s.data());
        ptrs.shrink_to_fit();
    }
    int argc() const { return (int)ptrs.size(); }
    char **argv() { return ptrs.data(); }
};

// graph_builder's chain for the options under test; -> the unknown argument, or "" if every argument was taken
struct Parsed {
    bool clipTips = false, simplify = false, popBubbles = false, autoRounds = false, walkAuto = false, rangeAuto = false;
    uint64_t tipMaxLen = 0;
    uint32_t maxDiff = 3;
    int rounds = 3, cutoff = -1, lo = 180, hi = 250;
    std::string out;
    ContigOpts contig;
    RankOpts ranks;
    std::string unknown;
    explicit Parsed(std::initializer_list<const char *> w) {
        Argv av(w);
        for (Args a(av.argc(), av.argv(), 0); a.more(); a.next()) {
            if (a.optional("--clip-tips", tipMaxLen)) clipTips = true;
            else if (a.optional("--pop-bubbles", maxDiff)) popBubbles = true;
            else if (a.flag("--simplify")) simplify = true;
            else if (a.word("--rounds", 1, "auto")) { autoRounds = true; a.skip(); }
            else if (a.value("--rounds", rounds)) autoRounds = false;
            else if (a.word("--walk-pairs", 2, "auto")) { a.value("--walk-pairs", cutoff); walkAuto = true; a.skip(); }
            else if (a.value("--walk-pairs", cutoff, lo, hi)) {}
            else if (a.word("--range", 1, "auto")) { rangeAuto = true; a.skip(); }
            else if (a.value("--range", lo, hi)) {}
            else if (a.value("--out", out) || contig.parse(a) || ranks.parse(a)) {}
            else { unknown = a.cur(); return; }
        }
    }
};

static void optionalValues() {
    { Parsed p({"--clip-tips", "auto"}); CHECK(p.clipTips && p.tipMaxLen == 0 && p.unknown.empty()); }
    { Parsed p({"--clip-tips", "40"}); CHECK(p.clipTips && p.tipMaxLen == 40 && p.unknown.empty()); }
    { Parsed p({"--clip-tips", "--simplify"}); CHECK(p.clipTips && p.tipMaxLen == 0 && p.simplify && p.unknown.empty()); }
    { Parsed p({"--clip-tips"}); CHECK(p.clipTips && p.tipMaxLen == 0 && p.unknown.empty()); }
    { Parsed p({"--clip-tips", "40", "--clip-tips", "auto"}); CHECK(p.tipMaxLen == 40); }            // auto leaves the value as it is
    { Parsed p({"--clip-tips", "x"}); CHECK(p.clipTips && p.unknown == "x"); }                       // not a value: the next argument
    { Parsed p({"--pop-bubbles", "5", "--simplify"}); CHECK(p.popBubbles && p.maxDiff == 5 && p.simplify); }
    { Parsed p({"--pop-bubbles", "auto", "--clip-tips", "7"}); CHECK(p.popBubbles && p.maxDiff == 3 && p.tipMaxLen == 7); }
}

static void multiValues() {
    { Parsed p({"--range", "100", "300"}); CHECK(!p.rangeAuto && p.lo == 100 && p.hi == 300 && p.unknown.empty()); }
    { Parsed p({"--range", "auto"}); CHECK(p.rangeAuto && p.lo == 180 && p.hi == 250 && p.unknown.empty()); }
    { Parsed p({"--range", "100"}); CHECK(p.unknown == "--range" && p.lo == 180); }
    { Parsed p({"--range"}); CHECK(p.unknown == "--range"); }
    { Parsed p({"--walk-pairs", "2", "100", "300"}); CHECK(!p.walkAuto && p.cutoff == 2 && p.lo == 100 && p.hi == 300 && p.unknown.empty()); }
    { Parsed p({"--walk-pairs", "2", "auto"}); CHECK(p.walkAuto && p.cutoff == 2 && p.lo == 180 && p.unknown.empty()); }
    { Parsed p({"--walk-pairs", "2", "auto", "--simplify"}); CHECK(p.walkAuto && p.simplify && p.unknown.empty()); }
    { Parsed p({"--walk-pairs", "2", "100"}); CHECK(p.unknown == "--walk-pairs" && p.cutoff == -1); }
    { Parsed p({"--walk-pairs", "2"}); CHECK(p.unknown == "--walk-pairs"); }
    { Parsed p({"--walk-pairs"}); CHECK(p.unknown == "--walk-pairs"); }
    { Parsed p({"--out"}); CHECK(p.unknown == "--out"); }                                            // a missing value: unknown argument
    { Parsed p({"--out", "a", "--out"}); CHECK(p.out == "a" && p.unknown == "--out"); }
}

static void overrides() {
    { Parsed p({"--out", "a", "--out", "b"}); CHECK(p.out == "b"); }
    { Parsed p({"--rounds", "5", "--rounds", "auto"}); CHECK(p.autoRounds && p.rounds == 5); }
    { Parsed p({"--rounds", "auto", "--rounds", "5"}); CHECK(!p.autoRounds && p.rounds == 5); }
    { Parsed p({"--range", "1", "2", "--range", "3", "4"}); CHECK(p.lo == 3 && p.hi == 4); }
    { Parsed p({"--walk-pairs", "2", "auto", "--walk-pairs", "4", "1", "2"}); CHECK(p.walkAuto && p.cutoff == 4 && p.lo == 1 && p.hi == 2); }
}

static void groups() {
    { Parsed p({"--simplify"}); CHECK(p.contig.path.empty() && p.contig.minLen == 0 && p.contig.width == 60 && !p.contig.both && p.ranks.world == 0 && p.ranks.rank == 0); }
    { Parsed p({"--contigs", "c.fa", "--contig-min-len", "50", "--contig-width", "0", "--contig-both-strands"});
      CHECK(p.contig.path == "c.fa" && p.contig.minLen == 50 && p.contig.width == 0 && p.contig.both && p.unknown.empty()); }
    { Parsed p({"--contig-width"}); CHECK(p.unknown == "--contig-width"); }
    { Parsed p({"--world", "2", "--rank", "1", "--id-file", "id"}); CHECK(p.ranks.world == 2 && p.ranks.rank == 1 && p.ranks.idFile == "id" && p.ranks.check()); }
    CHECK(RankOpts().check());                                                                       // no --world: nothing to check
    std::fprintf(stderr, "(four lines about --world follow: the checks that must fail)\n");
    { Parsed p({"--world", "2"}); CHECK(!p.ranks.check()); }
    { Parsed p({"--world", "2", "--rank", "2", "--id-file", "id"}); CHECK(!p.ranks.check()); }
    { Parsed p({"--world", "2", "--rank", "-1", "--id-file", "id"}); CHECK(!p.ranks.check()); }
    { Parsed p({"--world", "-1", "--rank", "0", "--id-file", "id"}); CHECK(!p.ranks.check()); }
}

static void numbers() {
    int i = 7; long l = 7; uint32_t u = 7; uint64_t w = 7;
    CHECK(Args::number("0", i) && i == 0);
    CHECK(Args::number("-12", i) && i == -12);
    CHECK(Args::number("65535", l) && l == 65535);
    CHECK(Args::number("4294967295", u) && u == 4294967295u);
    CHECK(Args::number("18446744073709551615", w) && w == UINT64_MAX);
    i = 7; u = 7; w = 7;
    CHECK(!Args::number("", i) && !Args::number("abc", i) && !Args::number("12x", i) && !Args::number("1 ", i) && !Args::number("2147483648", i) && i == 7);
    CHECK(!Args::number("-1", u) && !Args::number("4294967296", u) && !Args::number("1.5", u) && u == 7);
    CHECK(!Args::number("-1", w) && !Args::number("18446744073709551616", w) && !Args::number("0x10", w) && w == 7);
}

static void renderers() {
    std::map<uint64_t, uint64_t> h;
    CHECK(jsonPairs(h) == "[]");
    h[3] = 4;
    CHECK(jsonPairs(h) == "[[3,4]]");
    h[UINT64_MAX] = 0; h[1] = 2;
    CHECK(jsonPairs(h) == "[[1,2],[3,4],[18446744073709551615,0]]");
    CHECK(jsonList(std::vector<uint64_t>{}) == "[]");
    CHECK(jsonList(std::vector<uint64_t>{5}) == "[5]");
    CHECK(jsonList(std::vector<uint64_t>{5, 0, UINT64_MAX}) == "[5,0,18446744073709551615]");
    CHECK(jsonList(std::vector<int>{-1, 2}) == "[-1,2]");
    const char *names[3] = {"a", "b", "c"};
    const uint64_t values[3] = {1, 2, UINT64_MAX};
    CHECK(jsonNamed(names, values, 0) == "");
    CHECK(jsonNamed(names, values, 1) == "\"a\":1");
    CHECK(jsonNamed(names, values, 3) == "\"a\":1,\"b\":2,\"c\":18446744073709551615");
    std::string s = "{";
    jsonPut(s);
    CHECK(s == "{");
    jsonPut(s, "k", 31);
    CHECK(s == "{\"k\":31");
    jsonPut(s, "n", (uint64_t)UINT64_MAX, "neg", -3, "u", (uint32_t)4000000000u, "yes", true, "no", false, "raw", "null", "list", jsonList(std::vector<uint64_t>{1, 2}));
    CHECK(s == "{\"k\":31,\"n\":18446744073709551615,\"neg\":-3,\"u\":4000000000,\"yes\":true,\"no\":false,\"raw\":null,\"list\":[1,2]");
    jsonPut(s, "o", jsonObject());
    CHECK(s.substr(s.size() - 7) == ",\"o\":{}");
    CHECK(jsonObject("a", 1) == "{\"a\":1}");
    CHECK(jsonObject("a", 1, "b", jsonObject("c", false)) == "{\"a\":1,\"b\":{\"c\":false}}");
}

int main() {
    optionalValues();
    multiValues();
    overrides();
    groups();
    numbers();
    renderers();
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("tool_common_check ok\n");
    return 0;
}
