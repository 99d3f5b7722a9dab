// rt_usda.cpp — the .usda text layer reader: lexer and recursive-descent parser (see rt_usd.h).
#include "rt_usd_internal.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>

namespace rt {
namespace usd {

namespace {

struct Tok {
    enum T { kEnd, kPunct, kIdent, kNum, kStr, kAsset, kPath, kErr } t = kEnd;
    std::string s;
    double v = 0.0;
};

class Lexer {
public:
    Lexer(const char* b, size_t n) : p_(b), e_(b + n) {}
    const Tok& peek(size_t k = 0) {
        while (buf_.size() <= k) buf_.push_back(lex());
        return buf_[k];
    }
    Tok next() {
        peek();
        Tok t = std::move(buf_.front());
        buf_.pop_front();
        return t;
    }
    int line() const { return line_; }

private:
    const char* p_;
    const char* e_;
    int line_ = 1;
    std::deque<Tok> buf_;

    static bool ident_start(char c) { return std::isalpha((unsigned char)c) || c == '_'; }
    static bool ident_char(char c) { return std::isalnum((unsigned char)c) || c == '_'; }

    Tok lex() {
        Tok t;
        while (p_ < e_) {
            if (*p_ == '\n') { ++line_; ++p_; }
            else if (std::isspace((unsigned char)*p_)) ++p_;
            else if (*p_ == '#') { while (p_ < e_ && *p_ != '\n') ++p_; }
            else break;
        }
        if (p_ >= e_) return t;
        const char c = *p_;
        if (std::strchr("()[]{}=,:;", c)) {
            t.t = Tok::kPunct;
            t.s = std::string(1, c);
            ++p_;
            return t;
        }
        if (c == '"' || c == '\'') {
            const bool triple = e_ - p_ >= 3 && p_[1] == c && p_[2] == c;
            p_ += triple ? 3 : 1;
            t.t = Tok::kStr;
            while (p_ < e_) {
                if (triple ? (e_ - p_ >= 3 && p_[0] == c && p_[1] == c && p_[2] == c) : *p_ == c) {
                    p_ += triple ? 3 : 1;
                    return t;
                }
                if (*p_ == '\\' && p_ + 1 < e_) {
                    const char x = p_[1];
                    t.s += x == 'n' ? '\n' : x == 't' ? '\t' : x;
                    p_ += 2;
                    continue;
                }
                if (*p_ == '\n') ++line_;
                t.s += *p_++;
            }
            t.t = Tok::kErr;
            return t;
        }
        if (c == '@') {
            const bool triple = e_ - p_ >= 3 && p_[1] == '@' && p_[2] == '@';
            p_ += triple ? 3 : 1;
            t.t = Tok::kAsset;
            while (p_ < e_) {
                if (triple ? (e_ - p_ >= 3 && p_[0] == '@' && p_[1] == '@' && p_[2] == '@') : *p_ == '@') {
                    p_ += triple ? 3 : 1;
                    return t;
                }
                t.s += *p_++;
            }
            t.t = Tok::kErr;
            return t;
        }
        if (c == '<') {
            ++p_;
            t.t = Tok::kPath;
            while (p_ < e_ && *p_ != '>') t.s += *p_++;
            if (p_ >= e_) { t.t = Tok::kErr; return t; }
            ++p_;
            return t;
        }
        const bool sign = (c == '-' || c == '+') && p_ + 1 < e_;
        const char c1 = sign ? p_[1] : c;
        if (std::isdigit((unsigned char)c1) || (c1 == '.' && p_ + (sign ? 2 : 1) < e_ && std::isdigit((unsigned char)p_[sign ? 2 : 1]))) {
            char* end = nullptr;
            t.v = std::strtod(p_, &end);
            if (!end || end == p_) { t.t = Tok::kErr; return t; }
            t.t = Tok::kNum;
            p_ = end;
            return t;
        }
        if (sign && e_ - p_ >= 4 && !std::strncmp(p_ + 1, "inf", 3)) {
            t.t = Tok::kNum;
            t.v = c == '-' ? -INFINITY : INFINITY;
            p_ += 4;
            return t;
        }
        if (ident_start(c)) {
            t.t = Tok::kIdent;
            // names: a:b:c, optionally followed by .timeSamples / .connect (property suffixes)
            while (p_ < e_ && (ident_char(*p_) || ((*p_ == ':' || *p_ == '.') && p_ + 1 < e_ && ident_start(p_[1]))))
                t.s += *p_++;
            return t;
        }
        t.t = Tok::kErr;
        t.s = std::string(1, c);
        return t;
    }
};

class UsdaParser {
public:
    UsdaParser(const char* b, size_t n, Stage& st) : lx_(b, n), st_(st) {}
    bool run(std::string& err) {
        if (lx_.peek().t == Tok::kPunct && lx_.peek().s == "(") {
            if (!layer_meta()) return fail(err);
        }
        while (lx_.peek().t != Tok::kEnd) {
            if (!is_ident({"def", "over", "class"})) { msg_ = "expected a prim"; return fail(err); }
            if (!prim(0)) return fail(err);
        }
        return true;
    }

private:
    Lexer lx_;
    Stage& st_;
    std::string msg_;

    bool fail(std::string& err) {
        err = "usda line " + std::to_string(lx_.line()) + ": " + (msg_.empty() ? "syntax error" : msg_);
        return false;
    }
    bool is_punct(const char* s, size_t k = 0) { const Tok& t = lx_.peek(k); return t.t == Tok::kPunct && t.s == s; }
    bool is_ident(std::initializer_list<const char*> names, size_t k = 0) {
        const Tok& t = lx_.peek(k);
        if (t.t != Tok::kIdent) return false;
        for (const char* n : names)
            if (t.s == n) return true;
        return false;
    }
    bool expect(const char* p) {
        if (!is_punct(p)) { msg_ = std::string("expected '") + p + "'"; return false; }
        lx_.next();
        return true;
    }
    // skips a balanced (...), [...] or {...} group starting at the current token
    bool skip_group() {
        int depth = 0;
        do {
            Tok t = lx_.next();
            if (t.t == Tok::kEnd || t.t == Tok::kErr) { msg_ = "unbalanced group"; return false; }
            if (t.t == Tok::kPunct && (t.s == "(" || t.s == "[" || t.s == "{")) ++depth;
            if (t.t == Tok::kPunct && (t.s == ")" || t.s == "]" || t.s == "}")) --depth;
        } while (depth > 0);
        return true;
    }

    // nesting of values and prims is bounded: hostile input must not exhaust the stack
    static constexpr int kMaxDepth = 64;
    int depth_ = 0;
    struct Nest {
        int& d;
        explicit Nest(int& d_) : d(d_) { ++d; }
        ~Nest() { --d; }
    };

    bool value(Value& v) {
        Nest nest(depth_);
        if (depth_ > kMaxDepth) { msg_ = "values nested too deeply"; return false; }
        const Tok& t = lx_.peek();
        if (t.t == Tok::kPunct && t.s == "[") {
            lx_.next();
            v.array = true;
            bool first = true;
            while (!is_punct("]")) {
                Value el;
                if (!value(el)) return false;
                if (el.kind == Value::kNum) {
                    if (first) v.comps = (int)el.num.size();
                    v.kind = Value::kNum;
                    v.num.insert(v.num.end(), el.num.begin(), el.num.end());
                } else if (el.kind == Value::kStr || el.kind == Value::kPath) {
                    v.kind = el.kind;
                    v.str.insert(v.str.end(), el.str.begin(), el.str.end());
                }
                first = false;
                if (is_punct(",")) lx_.next();
                else if (!is_punct("]")) { msg_ = "expected ',' or ']'"; return false; }
            }
            lx_.next();
            if (v.kind == Value::kNone) v.kind = Value::kNum;   // empty array
            return true;
        }
        if (t.t == Tok::kPunct && t.s == "(") {
            lx_.next();
            while (!is_punct(")")) {
                Value el;
                if (!value(el)) return false;
                if (el.kind == Value::kNum) {
                    v.kind = Value::kNum;
                    v.num.insert(v.num.end(), el.num.begin(), el.num.end());
                } else if (el.kind != Value::kNone) {
                    v.kind = el.kind;
                    v.str.insert(v.str.end(), el.str.begin(), el.str.end());
                }
                if (is_punct(",")) lx_.next();
                else if (!is_punct(")")) { msg_ = "expected ',' or ')'"; return false; }
            }
            lx_.next();
            v.comps = v.kind == Value::kNum ? (int)v.num.size() : 1;
            return true;
        }
        if (t.t == Tok::kPunct && t.s == "{") return skip_group();   // dictionaries
        Tok x = lx_.next();
        switch (x.t) {
        case Tok::kNum: v.kind = Value::kNum; v.num.push_back(x.v); return true;
        case Tok::kStr:
        case Tok::kAsset: v.kind = Value::kStr; v.str.push_back(x.s); return true;
        case Tok::kPath: v.kind = Value::kPath; v.str.push_back(x.s); return true;
        case Tok::kIdent:
            if (x.s == "true" || x.s == "false") { v.kind = Value::kNum; v.num.push_back(x.s == "true" ? 1.0 : 0.0); return true; }
            if (x.s == "None") { v.kind = Value::kNone; return true; }
            if (x.s == "inf" || x.s == "nan") { v.kind = Value::kNum; v.num.push_back(x.s == "inf" ? INFINITY : NAN); return true; }
            v.kind = Value::kStr;
            v.str.push_back(x.s);
            return true;
        default: msg_ = "bad value"; return false;
        }
    }

    // a reference / payload / sublayer list: None, one item or [items]; an item is @asset@, </path>
    // or @asset@</path>, optionally followed by a (layer offset / custom data) group
    bool arc_list(std::vector<Arc>& out) {
        if (is_ident({"None"})) { lx_.next(); return true; }
        const bool list = is_punct("[");
        if (list) lx_.next();
        while (!(list && is_punct("]"))) {
            Arc a;
            if (lx_.peek().t == Tok::kAsset) a.asset = lx_.next().s;
            if (lx_.peek().t == Tok::kPath) a.path = lx_.next().s;
            else if (a.asset.empty()) { msg_ = "expected a reference"; return false; }
            if (is_punct("(") && !skip_group()) return false;
            out.push_back(a);
            if (!list) return true;
            if (is_punct(",")) lx_.next();
            else if (!is_punct("]")) { msg_ = "expected ',' or ']'"; return false; }
        }
        lx_.next();
        return true;
    }
    // variants = { string set = "variant" ... }
    bool variant_selection(int id) {
        if (!expect("{")) return false;
        while (!is_punct("}")) {
            if (is_punct(";")) { lx_.next(); continue; }
            if (lx_.peek().t == Tok::kIdent && lx_.peek(1).t != Tok::kPunct) lx_.next();   // value type
            const Tok set = lx_.next();
            if (set.t != Tok::kIdent && set.t != Tok::kStr) { msg_ = "expected a variant set name"; return false; }
            if (!expect("=")) return false;
            const Tok var = lx_.next();
            if (var.t != Tok::kStr) { msg_ = "expected a variant name"; return false; }
            st_.prims[id].variant_sel[set.s] = var.s;
        }
        lx_.next();
        return true;
    }

    // arcs_for: -2 plain metadata, -1 the layer's (subLayers), >= 0 a prim's (references, payload,
    // variants)
    bool meta_entries(const std::function<void(const std::string&, const Value&)>& on, int arcs_for = -2) {
        if (!expect("(")) return false;
        while (!is_punct(")")) {
            const Tok& t = lx_.peek();
            if (t.t == Tok::kStr) { lx_.next(); continue; }   // doc string
            if (t.t == Tok::kPunct && t.s == ";") { lx_.next(); continue; }
            if (t.t != Tok::kIdent) { msg_ = "bad metadata"; return false; }
            std::string op;
            if (is_ident({"prepend", "append", "add", "delete", "reorder"}) && lx_.peek(1).t == Tok::kIdent) op = lx_.next().s;
            std::string key = lx_.next().s;
            if (lx_.peek().t == Tok::kIdent && !is_punct("=")) key = lx_.next().s;   // typed dictionary entry
            if (!expect("=")) return false;
            if (arcs_for >= -1 && (key == "references" || key == "payload" || key == "subLayers" || key == "inherits" ||
                                   key == "specializes")) {
                std::vector<Arc> arcs;
                if (!arc_list(arcs)) return false;
                if (op == "delete" || op == "reorder") continue;
                if (arcs_for == -1 && key == "subLayers")
                    for (const Arc& a : arcs) st_.sublayers.push_back(a.asset);
                if (arcs_for >= 0 && key == "references") {
                    auto& r = st_.prims[arcs_for].references;
                    r.insert(op == "prepend" ? r.begin() : r.end(), arcs.begin(), arcs.end());
                }
                if (arcs_for >= 0 && key == "payload") {
                    auto& r = st_.prims[arcs_for].payloads;
                    r.insert(op == "prepend" ? r.begin() : r.end(), arcs.begin(), arcs.end());
                }
                continue;   // inherits / specializes: class arcs, not followed
            }
            if (arcs_for >= 0 && key == "variants") {
                if (!variant_selection(arcs_for)) return false;
                continue;
            }
            Value v;
            if (!value(v)) return false;
            on(key, v);
        }
        lx_.next();
        return true;
    }

    bool layer_meta() {
        return meta_entries([this](const std::string& k, const Value& v) {
            if (k == "upAxis" && v.kind == Value::kStr && !v.str.empty()) st_.up_axis = v.str[0];
            if (k == "defaultPrim" && v.kind == Value::kStr && !v.str.empty()) st_.default_prim = v.str[0];
            if ((k == "timeCodesPerSecond" || k == "framesPerSecond") && v.kind == Value::kNum && !v.num.empty()) {
                if (k == "timeCodesPerSecond" || !tcps_set_) st_.time_codes_per_second = v.num[0];
                if (k == "timeCodesPerSecond") tcps_set_ = true;
            }
        }, -1);
    }
    bool tcps_set_ = false;

    bool prim(int parent) {
        Nest nest(depth_);
        if (depth_ > kMaxDepth) { msg_ = "prims nested too deeply"; return false; }
        lx_.next();   // specifier
        std::string type;
        if (lx_.peek().t == Tok::kIdent) type = lx_.next().s;
        if (lx_.peek().t != Tok::kStr) { msg_ = "expected a prim name"; return false; }
        const std::string name = lx_.next().s;
        const int id = st_.add_prim(parent, name);
        if (!type.empty()) st_.prims[id].type = type;
        if (is_punct("(") && !prim_meta(id)) return false;
        return prim_body(id);
    }
    bool prim_meta(int id) {
        return meta_entries([this, id](const std::string& k, const Value& v) {
            Prim& p = st_.prims[id];
            if (k == "apiSchemas")
                for (const auto& s : v.str) p.api_schemas.push_back(s);
            if (k == "active" && v.kind == Value::kNum && !v.num.empty()) p.active = v.num[0] != 0.0;
        }, id);
    }
    // { properties, child prims, variant sets } of prim id (or of a variant body)
    bool prim_body(int id) {
        if (!expect("{")) return false;
        while (!is_punct("}")) {
            if (lx_.peek().t == Tok::kEnd) { msg_ = "unterminated prim"; return false; }
            if (is_ident({"def", "over", "class"})) {
                if (!prim(id)) return false;
            } else if (is_ident({"variantSet"})) {
                // variantSet "set" = { "variant" (metadata) { body } ... }: each body is kept as a
                // detached prim "/Prim{set=variant}"; load_stage applies the selected one
                Nest nest(depth_);
                if (depth_ > kMaxDepth) { msg_ = "prims nested too deeply"; return false; }
                lx_.next();
                const Tok set = lx_.next();
                if (set.t != Tok::kStr) { msg_ = "expected a variant set name"; return false; }
                if (!expect("=") || !expect("{")) return false;
                while (!is_punct("}")) {
                    const Tok var = lx_.next();
                    if (var.t != Tok::kStr) { msg_ = "expected a variant name"; return false; }
                    const int body = st_.add_detached(st_.prims[id].path + "{" + set.s + "=" + var.s + "}");
                    st_.prims[id].variant_bodies[set.s][var.s] = body;
                    if (is_punct("(") && !prim_meta(body)) return false;
                    if (!prim_body(body)) return false;
                }
                lx_.next();
            } else if (is_ident({"reorder"})) {
                lx_.next();
                lx_.next();
                if (!expect("=")) return false;
                Value v;
                if (!value(v)) return false;
            } else if (is_punct(";")) {
                lx_.next();
            } else if (!property(id)) {
                return false;
            }
        }
        lx_.next();
        return true;
    }

    bool property(int id) {
        bool uniform = false;
        while (is_ident({"custom", "uniform", "varying", "config", "prepend", "append", "add", "delete"})) {
            if (lx_.peek().s == "uniform") uniform = true;
            lx_.next();
        }
        if (lx_.peek().t != Tok::kIdent) { msg_ = "expected a property"; return false; }
        if (lx_.peek().s == "rel") {
            lx_.next();
            if (lx_.peek().t != Tok::kIdent) { msg_ = "expected a relationship name"; return false; }
            std::string name = lx_.next().s;
            auto& targets = st_.prims[id].rels[name];
            if (is_punct("=")) {
                lx_.next();
                Value v;
                if (!value(v)) return false;
                if (v.kind == Value::kPath) targets = v.str;
            }
            if (is_punct("(") && !meta_entries([](const std::string&, const Value&) {})) return false;
            return true;
        }
        std::string type = lx_.next().s;
        if (is_punct("[") && is_punct("]", 1)) {
            lx_.next();
            lx_.next();
            type += "[]";
        }
        if (lx_.peek().t != Tok::kIdent) { msg_ = "expected an attribute name"; return false; }
        std::string name = lx_.next().s;
        bool ts = false, conn = false;
        auto strip = [&name](const char* suf) {
            const size_t n = std::strlen(suf);
            if (name.size() > n && name.compare(name.size() - n, n, suf) == 0) { name.resize(name.size() - n); return true; }
            return false;
        };
        if (strip(".timeSamples")) ts = true;
        else if (strip(".connect")) conn = true;
        else strip(".spline");
        Attr& a = st_.prims[id].attrs[name];
        a.type = type;
        a.uniform = a.uniform || uniform;
        if (is_punct("=")) {
            lx_.next();
            if (ts) {
                if (!expect("{")) return false;
                while (!is_punct("}")) {
                    Tok k = lx_.next();
                    if (k.t != Tok::kNum) { msg_ = "expected a time code"; return false; }
                    if (!expect(":")) return false;
                    Value v;
                    if (!value(v)) return false;
                    a.times.push_back(k.v);
                    a.samples.push_back(v);
                    if (is_punct(",")) lx_.next();
                }
                lx_.next();
            } else if (conn) {
                Value v;
                if (!value(v)) return false;
                if (v.kind == Value::kPath) a.connections = v.str;
            } else {
                Value v;
                if (!value(v)) return false;
                if (v.kind != Value::kNone) {
                    a.value = v;
                    a.has_default = true;
                }
            }
        }
        if (is_punct("(")) {
            if (!meta_entries([&a](const std::string& k, const Value& v) {
                    if (k == "interpolation" && v.kind == Value::kStr && !v.str.empty()) a.interpolation = v.str[0];
                    if (k == "elementSize" && v.kind == Value::kNum && !v.num.empty()) a.element_size = element_size(v.num[0]);
                }))
                return false;
        }
        return true;
    }
};

}  // namespace

bool parse_usda(const char* text, size_t n, Stage& st, std::string& err) {
    UsdaParser p(text, n, st);
    return p.run(err);
}

}  // namespace usd
}  // namespace rt
