// Load sink for native health probes: a single-threaded epoll accept
// loop on 127.0.0.1:0 that prints its port on stdout and counts the
// connections it accepted. Stand-alone (no cpilot libs) so it costs the
// box as little as possible next to the daemon it is measuring.
//
// usage: cpilot_probesink MODE
//   accept   accept and wait for the peer to close
//   http200  answer any request with 200
//   http503  answer any request with 503
//   hang     read the request, never reply
//   split    answer 200 with the status line in 1-byte writes
//   close    close immediately without replying
//
// The accepted count is printed as {"accepted": N} on SIGTERM/SIGINT, and
// is the body of the reply to `GET /__sink/stats` (every mode but
// `close`, which never reads). Stats connections are not counted.
#include <arpa/inet.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <signal.h>
#include <sys/epoll.h>
#include <sys/resource.h>
#include <sys/signalfd.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

namespace {

enum class Mode { Accept, Http200, Http503, Hang, Split, Close };

struct Conn {
  std::string in;    // request bytes seen so far (bounded)
  std::string out;   // reply bytes still to write
  size_t chunk = 0;  // max bytes per write (0 = as much as fits)
  bool replied = false;
};

constexpr size_t kMaxRequest = 8192;
const char kStatsRequest[] = "GET /__sink/stats ";

int epfd = -1;
std::map<int, Conn> conns;
unsigned long long accepted = 0;

void watch(int fd, uint32_t events, int op) {
  struct epoll_event ev;
  memset(&ev, 0, sizeof(ev));
  ev.events = events;
  ev.data.fd = fd;
  epoll_ctl(epfd, op, fd, &ev);
}

void drop(int fd) {
  epoll_ctl(epfd, EPOLL_CTL_DEL, fd, nullptr);
  close(fd);
  conns.erase(fd);
}

std::string httpReply(int code, const char* text, const std::string& body) {
  return "HTTP/1.1 " + std::to_string(code) + " " + text +
         "\r\nContent-Type: text/plain\r\nContent-Length: " +
         std::to_string(body.size()) + "\r\nConnection: close\r\n\r\n" + body;
}

void startReply(int fd, Conn& c, std::string reply, size_t chunk) {
  c.out = std::move(reply);
  c.chunk = chunk;
  c.replied = true;
  watch(fd, EPOLLIN | EPOLLOUT, EPOLL_CTL_MOD);
}

// returns false when the connection was dropped
bool flush(int fd, Conn& c) {
  while (!c.out.empty()) {
    size_t want = c.chunk ? c.chunk : c.out.size();
    ssize_t n = send(fd, c.out.data(), want, MSG_NOSIGNAL);
    if (n > 0) {
      c.out.erase(0, (size_t)n);
      if (c.chunk) return true;  // one small write per wakeup
    } else if (n < 0 && errno == EINTR) {
      continue;
    } else if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) {
      return true;
    } else {
      drop(fd);
      return false;
    }
  }
  drop(fd);  // reply complete
  return false;
}

void onRequestBytes(int fd, Conn& c, Mode mode) {
  if (c.replied) return;
  static const size_t kStatsLen = sizeof(kStatsRequest) - 1;
  if (c.in.compare(0, kStatsLen, kStatsRequest) == 0) {
    accepted--;  // a stats connection is not load
    startReply(fd, c,
               httpReply(200, "OK",
                         "{\"accepted\": " + std::to_string(accepted) + "}\n"),
               0);
    return;
  }
  if (c.in.find("\r\n\r\n") == std::string::npos) return;
  switch (mode) {
    case Mode::Http200:
      startReply(fd, c, httpReply(200, "OK", "ok\n"), 0);
      break;
    case Mode::Http503:
      startReply(fd, c, httpReply(503, "Service Unavailable", "down\n"), 0);
      break;
    case Mode::Split:
      startReply(fd, c, httpReply(200, "OK", "ok\n"), 1);
      break;
    default:
      break;  // accept, hang: never reply
  }
}

void onConn(int fd, uint32_t events, Mode mode) {
  auto it = conns.find(fd);
  if (it == conns.end()) return;
  Conn& c = it->second;
  if (events & EPOLLIN) {
    char buf[4096];
    while (true) {
      ssize_t n = recv(fd, buf, sizeof(buf), 0);
      if (n > 0) {
        if (c.in.size() < kMaxRequest)
          c.in.append(buf, (size_t)n);
        onRequestBytes(fd, c, mode);
      } else if (n < 0 && errno == EINTR) {
        continue;
      } else if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) {
        break;
      } else {
        drop(fd);  // peer closed or reset
        return;
      }
    }
  } else if (events & (EPOLLERR | EPOLLHUP)) {
    drop(fd);
    return;
  }
  if ((events & EPOLLOUT) && !c.out.empty()) flush(fd, c);
}

void onListener(int lfd, Mode mode) {
  for (int i = 0; i < 1024; i++) {
    int fd = accept4(lfd, nullptr, nullptr, SOCK_NONBLOCK | SOCK_CLOEXEC);
    if (fd < 0) {
      if (errno == EINTR) continue;
      return;  // EAGAIN, or EMFILE: retry on the next wakeup
    }
    accepted++;
    if (mode == Mode::Close) {
      close(fd);
      continue;
    }
    int one = 1;
    setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
    conns.emplace(fd, Conn{});
    watch(fd, EPOLLIN, EPOLL_CTL_ADD);
  }
}

}  // namespace

int main(int argc, char** argv) {
  static const std::map<std::string, Mode> kModes = {
      {"accept", Mode::Accept},   {"http200", Mode::Http200},
      {"http503", Mode::Http503}, {"hang", Mode::Hang},
      {"split", Mode::Split},     {"close", Mode::Close}};
  if (argc != 2 || !kModes.count(argv[1])) {
    fprintf(stderr,
            "usage: %s accept|http200|http503|hang|split|close\n", argv[0]);
    return 2;
  }
  Mode mode = kModes.at(argv[1]);

  struct rlimit rl;
  if (getrlimit(RLIMIT_NOFILE, &rl) == 0 && rl.rlim_cur < rl.rlim_max) {
    rl.rlim_cur = rl.rlim_max;
    setrlimit(RLIMIT_NOFILE, &rl);
  }

  sigset_t mask;
  sigemptyset(&mask);
  sigaddset(&mask, SIGTERM);
  sigaddset(&mask, SIGINT);
  sigprocmask(SIG_BLOCK, &mask, nullptr);
  signal(SIGPIPE, SIG_IGN);
  int sfd = signalfd(-1, &mask, SFD_NONBLOCK | SFD_CLOEXEC);

  int lfd = socket(AF_INET, SOCK_STREAM | SOCK_NONBLOCK | SOCK_CLOEXEC, 0);
  struct sockaddr_in addr;
  memset(&addr, 0, sizeof(addr));
  addr.sin_family = AF_INET;
  addr.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
  addr.sin_port = 0;
  socklen_t alen = sizeof(addr);
  if (lfd < 0 || sfd < 0 ||
      bind(lfd, (struct sockaddr*)&addr, sizeof(addr)) != 0 ||
      listen(lfd, 4096) != 0 ||
      getsockname(lfd, (struct sockaddr*)&addr, &alen) != 0) {
    perror("probesink: listen on 127.0.0.1");
    return 1;
  }
  epfd = epoll_create1(EPOLL_CLOEXEC);
  if (epfd < 0) {
    perror("probesink: epoll_create1");
    return 1;
  }
  watch(lfd, EPOLLIN, EPOLL_CTL_ADD);
  watch(sfd, EPOLLIN, EPOLL_CTL_ADD);

  printf("%d\n", (int)ntohs(addr.sin_port));
  fflush(stdout);

  struct epoll_event events[256];
  while (true) {
    int n = epoll_wait(epfd, events, 256, -1);
    if (n < 0) {
      if (errno == EINTR) continue;
      perror("probesink: epoll_wait");
      return 1;
    }
    for (int i = 0; i < n; i++) {
      int fd = events[i].data.fd;
      if (fd == sfd) {
        printf("{\"accepted\": %llu}\n", accepted);
        fflush(stdout);
        return 0;
      }
      if (fd == lfd) onListener(lfd, mode);
      else onConn(fd, events[i].events, mode);
    }
  }
}
