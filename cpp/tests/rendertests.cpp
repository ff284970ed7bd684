// Tests for native watch rendering: the template engine against data
// (cpilot/tmpl.hpp), the health-entry parser and the data model handed to
// templates, the `watches[].render` config rules, and the atomic write
// helper (cpilot/watches.hpp). No daemon, no network; files live in a
// temporary directory that is removed at the end.
// Run via `bin/cpilot_rendertests`; exits non-zero if any check failed.
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "cpilot/config.hpp"
#include "cpilot/discovery.hpp"
#include "cpilot/json.hpp"
#include "cpilot/tmpl.hpp"
#include "cpilot/watches.hpp"

using namespace cpilot;

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                         \
    }                                                                     \
  } while (0)
#define CHECK_EQ(a, b)                                                    \
  do {                                                                    \
    auto va = (a);                                                        \
    auto vb = (b);                                                        \
    if (!(va == vb)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s != %s\n  got:  %s\n  want: %s\n",   \
              __FILE__, __LINE__, #a, #b, std::string(va).c_str(),        \
              std::string(vb).c_str());                                   \
      failures++;                                                         \
    }                                                                     \
  } while (0)

namespace {

std::string render(const std::string& tmpl, const std::string& dataJson) {
  return Template::parse(tmpl).render(parseJson5(dataJson));
}

// the what() of whatever rendering throws, "" when it does not throw
std::string renderError(const std::string& tmpl, const std::string& dataJson) {
  try {
    render(tmpl, dataJson);
  } catch (const std::exception& e) {
    return e.what();
  }
  return "";
}

// ---------- engine on data ----------

void testEngineOnData() {
  const std::string data =
      R"({"Name": "web", "Healthy": true, "Empty": false,
          "A": {"B": {"C": "deep"}, "N": 7},
          "Items": [{"Host": "h1", "Port": 81}, {"Host": "h2", "Port": 82}],
          "One": [{"Host": "only", "Port": 1}],
          "None": []})";

  // chained fields
  CHECK_EQ(render("{{ .Name }}", data), std::string("web"));
  CHECK_EQ(render("{{ .A.B.C }}/{{ .A.N }}", data), std::string("deep/7"));
  // a missing key yields "", at any depth
  CHECK_EQ(render("[{{ .Nope }}][{{ .A.Nope }}][{{ .A.Nope.More }}]", data),
           std::string("[][][]"));
  // a field on a string (or any non-map) yields ""
  CHECK_EQ(render("[{{ .Name.Field }}][{{ .A.N.Field }}]", data),
           std::string("[][]"));

  // $v.Field on assignment and range variables, chained too
  CHECK_EQ(render("{{ $a := .A }}{{ $a.N }}-{{ $a.B.C }}-[{{ $a.Nope }}]",
                  data),
           std::string("7-deep-[]"));
  CHECK_EQ(render("{{ range $v := .Items }}{{ $v.Host }};{{ end }}", data),
           std::string("h1;h2;"));
  CHECK_EQ(render("{{ range $i, $v := .Items }}{{ $i }}={{ $v.Host }}:"
                  "{{ $v.Port }} {{ end }}",
                  data),
           std::string("0=h1:81 1=h2:82 "));
  // "$" is the root inside a range
  CHECK_EQ(render("{{ range .Items }}{{ $.Name }}@{{ .Host }} {{ end }}",
                  data),
           std::string("web@h1 web@h2 "));

  // range over a list of maps sets "." to each map: 0, 1 and 2 items
  const std::string line = "{{ .Host }}:{{ .Port }};";
  CHECK_EQ(render("<{{ range .None }}" + line + "{{ end }}>", data),
           std::string("<>"));
  CHECK_EQ(render("<{{ range .One }}" + line + "{{ end }}>", data),
           std::string("<only:1;>"));
  CHECK_EQ(render("<{{ range .Items }}" + line + "{{ end }}>", data),
           std::string("<h1:81;h2:82;>"));

  // index on a map (also of a missing key), len on a map and a list
  CHECK_EQ(render(R"({{ index .A "N" }}[{{ index .A "Nope" }}])", data),
           std::string("7[]"));
  CHECK_EQ(render(R"({{ index (index .A "B") "C" }})", data),
           std::string("deep"));
  CHECK_EQ(render("{{ len .A }} {{ len .Items }} {{ len .None }}", data),
           std::string("2 2 0"));
  CHECK_EQ(render("{{ $second := index .Items 1 }}{{ $second.Host }}", data),
           std::string("h2"));

  // if on a bool, a list and a map
  CHECK_EQ(render("{{ if .Healthy }}up{{ else }}down{{ end }}", data),
           std::string("up"));
  CHECK_EQ(render("{{ if .Empty }}up{{ else }}down{{ end }}", data),
           std::string("down"));
  CHECK_EQ(render("{{ if .None }}some{{ else }}none{{ end }}", data),
           std::string("none"));
  CHECK_EQ(render("{{ with .A }}{{ .N }}{{ end }}", data), std::string("7"));

  // env and the other functions still work, and env reads the environment
  setenv("CPILOT_RENDERTEST_VAR", "from-env", 1);
  CHECK_EQ(render(R"({{ env "CPILOT_RENDERTEST_VAR" }}/{{ .Name }})", data),
           std::string("from-env/web"));
  // ... while "." no longer does
  CHECK_EQ(render("[{{ .CPILOT_RENDERTEST_VAR }}]", data), std::string("[]"));
  CHECK_EQ(render(R"({{ .Name | default "x" }} {{ .Nope | default "x" }})",
                  data),
           std::string("web x"));
  // and renderTemplate still renders against the environment
  CHECK_EQ(renderTemplate("{{ .CPILOT_RENDERTEST_VAR }}"),
           std::string("from-env"));
  // ... with the same lexing: `$v.Field` is a field of `$v` there too (a
  // field of a string renders empty), not `$v` with a stray token dropped
  CHECK_EQ(renderTemplate("{{ $v := .CPILOT_RENDERTEST_VAR }}{{ $v.Field }}"),
           std::string(""));
  CHECK_EQ(renderTemplate("{{ $v := .CPILOT_RENDERTEST_VAR }}{{ $v }}"),
           std::string("from-env"));

  // range over a map field that is not a list: the existing error
  CHECK_EQ(renderError("{{ range .Name }}x{{ end }}", data),
           std::string("template: range over non-list value"));
  CHECK_EQ(renderError("{{ range .A }}x{{ end }}", data),
           std::string("template: range over non-list value"));
  CHECK_EQ(renderError("{{ range .Nope }}x{{ end }}", data),
           std::string("template: range over non-list value"));

  // parse errors surface from parse(), not render()
  bool threw = false;
  try {
    Template::parse("{{ range .Items }}never closed");
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  // a never-parsed template refuses to render
  threw = false;
  try {
    Template().render(Json(JsonObject{}));
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
}

// ---------- parser and model ----------

const char* kUpstream =
    "{{ range .Services }}server {{ .Address }}:{{ .Port }}; # {{ .ID }}\n"
    "{{ end }}";

std::string renderBody(const std::string& tmpl, const std::string& body,
                       const std::string& tag = "", const std::string& dc = "") {
  bool ok = true;
  auto entries = parseHealthEntries(body, &ok);
  CHECK(ok);
  return Template::parse(tmpl).render(
      buildRenderData("backend", tag, dc, entries));
}

void testParserAndModel() {
  // two entries returned in reverse order render sorted
  const std::string reversed = R"([
    {"Node": {"Node": "n2", "Address": "192.168.0.2"},
     "Service": {"ID": "b-2", "Service": "backend", "Address": "10.0.0.2",
                 "Port": 9000, "Tags": ["blue", "v2"]}, "Checks": []},
    {"Node": {"Node": "n1", "Address": "192.168.0.1"},
     "Service": {"ID": "b-1", "Service": "backend", "Address": "10.0.0.1",
                 "Port": 9000, "Tags": []}, "Checks": []}])";
  CHECK_EQ(renderBody(kUpstream, reversed),
           std::string("server 10.0.0.1:9000; # b-1\n"
                       "server 10.0.0.2:9000; # b-2\n"));
  // same address: port, then ID, break the tie
  const std::string ties = R"([
    {"Service": {"ID": "z", "Address": "10.0.0.1", "Port": 2}},
    {"Service": {"ID": "b", "Address": "10.0.0.1", "Port": 1}},
    {"Service": {"ID": "a", "Address": "10.0.0.1", "Port": 1}}])";
  CHECK_EQ(renderBody("{{ range .Services }}{{ .ID }}{{ end }}", ties),
           std::string("abz"));

  // an empty Service.Address means the node's address, also for sorting
  const std::string fallback = R"([
    {"Node": {"Node": "n9", "Address": "10.0.0.9"},
     "Service": {"ID": "late", "Address": "10.0.0.5", "Port": 80}},
    {"Node": {"Node": "n3", "Address": "10.0.0.3"},
     "Service": {"ID": "onnode", "Address": "", "Port": 80}}])";
  CHECK_EQ(renderBody(kUpstream, fallback),
           std::string("server 10.0.0.3:80; # onnode\n"
                       "server 10.0.0.5:80; # late\n"));
  CHECK_EQ(renderBody("{{ range .Services }}{{ .Node }}/{{ .NodeAddress }} "
                      "{{ end }}",
                      fallback),
           std::string("n3/10.0.0.3 n9/10.0.0.9 "));

  // tags arrive as a list usable with join
  CHECK_EQ(renderBody("{{ range .Services }}[{{ join \",\" .Tags }}]"
                      "{{ len .Tags }}{{ end }}",
                      reversed),
           std::string("[]0[blue,v2]2"));

  // an entry without a Node object renders "" for .Node and .NodeAddress
  const std::string noNode =
      R"([{"Service": {"ID": "x", "Address": "10.1.1.1", "Port": 1}}])";
  CHECK_EQ(renderBody("{{ range .Services }}[{{ .Node }}][{{ .NodeAddress }}]"
                      "{{ .Address }}{{ end }}",
                      noNode),
           std::string("[][]10.1.1.1"));

  // the top of the model
  CHECK_EQ(renderBody("{{ .Name }}|{{ .Tag }}|{{ .DC }}|{{ .Healthy }}|"
                      "{{ len .Services }}|"
                      "{{ range .Services }}{{ .Name }}{{ end }}",
                      noNode, "blue", "dc1"),
           std::string("backend|blue|dc1|true|1|backend"));
  CHECK_EQ(renderBody("{{ .Name }}|{{ .Tag }}|{{ .DC }}|{{ .Healthy }}|"
                      "{{ len .Services }}",
                      "[]"),
           std::string("backend|||false|0"));

  // the parser keeps what change detection compares, unchanged
  bool ok = true;
  auto entries = parseHealthEntries(reversed, &ok);
  CHECK(ok);
  CHECK(entries.size() == 2);
  if (entries.size() == 2) {
    CHECK_EQ(entries[0].id, std::string("b-2"));
    CHECK_EQ(entries[0].address, std::string("10.0.0.2"));
    CHECK(entries[0].port == 9000);
    CHECK(entries[0].tags.size() == 2);
    CHECK_EQ(entries[0].node, std::string("n2"));
    CHECK_EQ(entries[0].nodeAddress, std::string("192.168.0.2"));
  }
  ok = true;
  parseHealthEntries("not json [", &ok);
  CHECK(!ok);
}

// ---------- config ----------

// decode `watches: [ {name: backend, interval: 3, <extra>} ]`
bool decodeWatch(const std::string& extra,
                 std::vector<std::shared_ptr<WatchConfig>>* out,
                 std::string* err) {
  Json raw = parseJson5("[{name: 'backend', interval: 3" +
                        (extra.empty() ? "" : ", " + extra) + "}]");
  return newWatchConfigs(raw, out, err);
}

void expectRejected(const std::string& render, const std::string& message) {
  std::vector<std::shared_ptr<WatchConfig>> out;
  std::string err;
  bool ok = decodeWatch("render: " + render, &out, &err);
  if (ok) {
    fprintf(stderr, "FAIL: accepted render: %s\n", render.c_str());
    failures++;
    return;
  }
  CHECK_EQ(err, message);
}

std::shared_ptr<RenderConfig> expectAccepted(const std::string& render) {
  std::vector<std::shared_ptr<WatchConfig>> out;
  std::string err;
  bool ok = decodeWatch("render: " + render, &out, &err);
  if (!ok || out.size() != 1 || !out[0]->render) {
    fprintf(stderr, "FAIL: rejected render: %s: %s\n", render.c_str(),
            err.c_str());
    failures++;
    return std::make_shared<RenderConfig>();
  }
  return out[0]->render;
}

void testConfig(const std::string& dir) {
  // a watch without render decodes as before
  {
    std::vector<std::shared_ptr<WatchConfig>> out;
    std::string err;
    CHECK(decodeWatch("tag: 'blue', dc: 'dc1', blocking: true", &out, &err));
    CHECK(out.size() == 1);
    if (out.size() == 1) {
      CHECK_EQ(out[0]->name, std::string("watch.backend"));
      CHECK_EQ(out[0]->serviceName, std::string("backend"));
      CHECK(out[0]->poll == 3);
      CHECK_EQ(out[0]->tag, std::string("blue"));
      CHECK_EQ(out[0]->dc, std::string("dc1"));
      CHECK(out[0]->blocking);
      CHECK(!out[0]->render);
      CHECK(loadRenderTemplate(*out[0], &err));  // nothing to load
    }
    CHECK(decodeWatch("render: null", &out, &err));
    CHECK(out.size() == 1 && !out[0]->render);
  }

  // accepted: the keys, the default mode
  auto r = expectAccepted("{source: '/t/in.ctmpl', dest: '/t/out.conf'}");
  CHECK_EQ(r->source, std::string("/t/in.ctmpl"));
  CHECK_EQ(r->dest, std::string("/t/out.conf"));
  CHECK(r->mode == 0644);
  CHECK(!r->tmpl.parsed());  // decoding never reads the file

  // unknown keys
  expectRejected("{source: '/a', dest: '/b', owner: 'root'}",
                 "watch[backend].render: invalid keys: owner");
  expectRejected("'/a'", "watch[backend].render must be an object");
  // required
  expectRejected("{dest: '/b'}", "watch[backend].render.source is required");
  expectRejected("{source: '/a'}", "watch[backend].render.dest is required");
  // non-empty
  expectRejected("{source: '', dest: '/b'}",
                 "watch[backend].render.source must be a non-empty string");
  expectRejected("{source: '/a', dest: ''}",
                 "watch[backend].render.dest must be a non-empty string");
  expectRejected("{source: '/a', dest: 7}",
                 "watch[backend].render.dest must be a non-empty string");
  // absolute
  expectRejected("{source: 'a.ctmpl', dest: '/b'}",
                 "watch[backend].render.source must be an absolute path");
  expectRejected("{source: '/a', dest: 'conf.d/b'}",
                 "watch[backend].render.dest must be an absolute path");
  // different
  expectRejected("{source: '/a', dest: '/a'}",
                 "watch[backend].render.dest must differ from source");
  // mode: octal, 0000-0777
  const std::string badMode =
      "watch[backend].render.mode must be an octal string from \"0000\" to "
      "\"0777\"";
  CHECK(expectAccepted("{source: '/a', dest: '/b', mode: '0600'}")->mode ==
        0600);
  CHECK(expectAccepted("{source: '/a', dest: '/b', mode: '0000'}")->mode == 0);
  CHECK(expectAccepted("{source: '/a', dest: '/b', mode: '0777'}")->mode ==
        0777);
  CHECK(expectAccepted("{source: '/a', dest: '/b', mode: '640'}")->mode ==
        0640);
  expectRejected("{source: '/a', dest: '/b', mode: '0888'}", badMode);
  expectRejected("{source: '/a', dest: '/b', mode: '1777'}", badMode);
  expectRejected("{source: '/a', dest: '/b', mode: 'rw-r--r--'}", badMode);
  expectRejected("{source: '/a', dest: '/b', mode: ''}", badMode);
  expectRejected("{source: '/a', dest: '/b', mode: 420}", badMode);

  // newConfig (text only) accepts a render whose source does not exist
  const std::string missing = dir + "/missing.ctmpl";
  auto configText = [&](const std::string& source) {
    return "{consul: 'localhost:8500', watches: [{name: 'backend', "
           "interval: 3, render: {source: '" +
           source + "', dest: '" + dir + "/out.conf'}}]}";
  };
  std::string err;
  CHECK(newConfig(configText(missing), &err) != nullptr);
  {
    std::string nerr;
    CHECK(newConfig("{consul: 'localhost:8500', watches: [{name: 'backend', "
                    "interval: 3, render: {source: 'rel', dest: '/b'}}]}",
                    &nerr) == nullptr);
    CHECK_EQ(nerr, std::string("unable to parse watches: watch[backend]."
                               "render.source must be an absolute path"));
  }

  // loadConfig reads and parses the source
  auto writeFile = [](const std::string& path, const std::string& text) {
    std::ofstream f(path, std::ios::binary);
    f << text;
  };
  const std::string cfgPath = dir + "/containerpilot.json5";
  writeFile(cfgPath, configText(missing));
  err.clear();
  CHECK(loadConfig(cfgPath, &err) == nullptr);
  CHECK_EQ(err, "watch[backend].render.source: open " + missing +
                    ": No such file or directory");

  const std::string bad = dir + "/bad.ctmpl";
  writeFile(bad, "{{ range .Services }}{{ .Address ");
  writeFile(cfgPath, configText(bad));
  err.clear();
  CHECK(loadConfig(cfgPath, &err) == nullptr);
  CHECK_EQ(err, std::string("watch[backend].render.source: template: "
                            "unclosed action"));

  const std::string good = dir + "/good.ctmpl";
  writeFile(good, "{{ len .Services }} up\n");
  writeFile(cfgPath, configText(good));
  err.clear();
  auto cfg = loadConfig(cfgPath, &err);
  CHECK(cfg != nullptr);
  if (cfg) {
    CHECK(cfg->watches.size() == 1 && cfg->watches[0]->render &&
          cfg->watches[0]->render->tmpl.parsed());
    CHECK_EQ(cfg->watches[0]->render->tmpl.render(
                 buildRenderData("backend", "", "", {})),
             std::string("0 up\n"));
  }
}

// ---------- atomic write helper ----------

std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

std::vector<std::string> listDir(const std::string& dir) {
  std::vector<std::string> names;
  DIR* d = opendir(dir.c_str());
  if (!d) return names;
  while (struct dirent* e = readdir(d)) {
    std::string n = e->d_name;
    if (n != "." && n != "..") names.push_back(n);
  }
  closedir(d);
  return names;
}

void testAtomicWrite(const std::string& root) {
  const std::string dir = root + "/out";
  CHECK(mkdir(dir.c_str(), 0755) == 0);
  const std::string dest = dir + "/upstreams.conf";
  std::string err;

  // creates the file with the requested mode, whatever the umask says
  mode_t old = umask(077);
  CHECK(writeFileAtomic(dest, "one\n", 0644, &err));
  umask(old);
  struct stat st1;
  CHECK(stat(dest.c_str(), &st1) == 0);
  CHECK((st1.st_mode & 07777) == 0644);
  CHECK_EQ(slurp(dest), std::string("one\n"));
  CHECK(listDir(dir).size() == 1);

  // identical bytes: same inode, same mtime
  struct timespec past[2] = {{1000000000, 0}, {1000000000, 0}};
  CHECK(utimensat(AT_FDCWD, dest.c_str(), past, 0) == 0);
  CHECK(writeFileAtomic(dest, "one\n", 0644, &err));
  struct stat st2;
  CHECK(stat(dest.c_str(), &st2) == 0);
  CHECK(st2.st_ino == st1.st_ino);
  CHECK(st2.st_mtim.tv_sec == 1000000000 && st2.st_mtim.tv_nsec == 0);

  // different bytes replace the file (a new inode: it was renamed over)
  CHECK(writeFileAtomic(dest, "two, longer\n", 0600, &err));
  struct stat st3;
  CHECK(stat(dest.c_str(), &st3) == 0);
  CHECK(st3.st_ino != st1.st_ino);
  CHECK((st3.st_mode & 07777) == 0600);
  CHECK(st3.st_mtim.tv_sec != 1000000000);
  CHECK_EQ(slurp(dest), std::string("two, longer\n"));
  // shorter content leaves no tail of the longer one
  CHECK(writeFileAtomic(dest, "", 0644, &err));
  CHECK_EQ(slurp(dest), std::string(""));
  CHECK(listDir(dir).size() == 1);

  // a missing directory: an error, and no temporary file anywhere
  err.clear();
  CHECK(!writeFileAtomic(root + "/nowhere/upstreams.conf", "x", 0644, &err));
  CHECK(err.find("No such file or directory") != std::string::npos);
  for (auto& name : listDir(root))
    CHECK(name.find(".tmp") == std::string::npos);
  CHECK(listDir(dir).size() == 1);

  // dest is a directory: rename fails, the temporary file is removed and
  // dest is left as it was
  const std::string blocked = dir + "/blocked";
  CHECK(mkdir(blocked.c_str(), 0755) == 0);
  err.clear();
  CHECK(!writeFileAtomic(blocked, "x", 0644, &err));
  CHECK(!err.empty());
  struct stat st4;
  CHECK(stat(blocked.c_str(), &st4) == 0 && S_ISDIR(st4.st_mode));
  CHECK(listDir(dir).size() == 2);  // upstreams.conf + blocked, no *.tmp.*
}

}  // namespace

int main() {
  char tmpl[] = "/tmp/cpilot-rendertests-XXXXXX";
  const char* root = mkdtemp(tmpl);
  if (!root) {
    perror("mkdtemp");
    return 1;
  }
  testEngineOnData();
  testParserAndModel();
  testConfig(root);
  testAtomicWrite(root);
  std::string cleanup = std::string("rm -rf '") + root + "'";
  if (system(cleanup.c_str()) != 0) perror("cleanup");

  if (failures) {
    fprintf(stderr, "%d render test check(s) failed\n", failures);
    return 1;
  }
  printf("all render tests passed\n");
  return 0;
}
