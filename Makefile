# binder-amd: native-first rebuild of TritonDataCenter/binder.
# Everything is plain C++20 + POSIX; no external libraries.

CXX ?= g++
PYTHON ?= python3
CXXFLAGS ?= -O2 -g -std=c++20 -fPIC -fno-omit-frame-pointer \
	-Wall -Wextra -Werror -Wno-unused-parameter -MMD -MP
LDFLAGS ?=

BUILD := build

CORE_SRCS := \
	native/common/json.cpp \
	native/common/log.cpp \
	native/common/loop.cpp \
	native/dns/codec.cpp \
	native/engine/store.cpp \
	native/engine/engine.cpp

SERVER_SRCS := \
	native/server/metrics.cpp \
	native/server/server.cpp \
	native/server/recursion.cpp \
	native/server/ldap.cpp \
	native/zk/client.cpp \
	native/zk/mirror.cpp

CORE_OBJS := $(CORE_SRCS:%.cpp=$(BUILD)/%.o)
SERVER_OBJS := $(SERVER_SRCS:%.cpp=$(BUILD)/%.o)

PY_EXT_SUFFIX := $(shell $(PYTHON)-config --extension-suffix 2>/dev/null || echo .so)
PY_INCLUDES := $(shell $(PYTHON) -m pybind11 --includes)
PYMOD := binder_amd/_native$(PY_EXT_SUFFIX)

BINARIES := bin/binderd bin/binder-balancer bin/dnsblast bin/bsockblast \
	bin/binder-adjust bin/binder-supervisor bin/zklogcat bin/zktool \
	bin/zkd

all: $(PYMOD) $(BINARIES)

bin/binderd: $(CORE_OBJS) $(SERVER_OBJS) $(BUILD)/native/server/binderd_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS) -lssl -lcrypto -lpthread

bin/binder-balancer: $(CORE_OBJS) $(BUILD)/native/balancer/balancer_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS)

bin/dnsblast: $(CORE_OBJS) $(BUILD)/native/bench/dnsblast_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS) -lpthread

bin/bsockblast: $(CORE_OBJS) $(BUILD)/native/bench/bsockblast_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS)

bin/binder-adjust: $(CORE_OBJS) $(BUILD)/native/adjust/adjust_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS)

bin/binder-supervisor: $(CORE_OBJS) $(BUILD)/native/adjust/supervisor_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS)

bin/zklogcat: $(CORE_OBJS) $(BUILD)/native/zklog/zklogcat_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS)

bin/zktool: $(CORE_OBJS) $(BUILD)/native/zk/client.o $(BUILD)/native/zk/zktool_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS)

bin/zkd: $(CORE_OBJS) $(BUILD)/native/zkd/zkd_main.o
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) $^ -o $@ $(LDFLAGS)

$(BUILD)/%.o: %.cpp
	@mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -c $< -o $@

# pybind11 module (compiled separately: needs Python includes, and
# -Wno-error for pybind's warnings under -Wextra)
$(BUILD)/native/pybind/module.o: native/pybind/module.cpp
	@mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -Wno-error $(PY_INCLUDES) -c $< -o $@

$(PYMOD): $(CORE_OBJS) $(BUILD)/native/pybind/module.o
	$(CXX) -shared $(CXXFLAGS) $^ -o $@ $(LDFLAGS)

# `make test` parity with the reference's nodeunit target
# (Makefile:169-171 there)
test: all
	$(PYTHON) -m pytest tests -q -m "not gpu"

# Lint/style gate (parity with the reference's eslint/jsstyle/cstyle
# gates, /root/reference/Makefile:17-20): C++ and Python style checks in
# tools/lint.py; -Werror already covers compiler diagnostics.
check: all
	$(PYTHON) -m py_compile binder_amd/*.py bench.py __graft_entry__.py
	$(PYTHON) tools/lint.py
	@echo "check OK"

# Sanitizer run of the balancer-socket receive buffer (framebuf.hpp) in
# a stand-alone program: random frame streams, random split points, one
# maximum-size frame. Host-only, CPU-only.
$(BUILD)/framebuf_check: native/server/framebuf_check_main.cpp \
		native/server/framebuf.hpp native/balancer/protocol.hpp
	@mkdir -p $(BUILD)
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -Werror \
	    -fsanitize=address,undefined -fno-sanitize-recover=all \
	    $< -o $@

check-framebuf: $(BUILD)/framebuf_check
	$(BUILD)/framebuf_check 1 40

# Sanitizer run of the answer table (answertab.hpp) in a stand-alone
# program: a seeded random operation sequence against a std::unordered_map
# model, with masked (colliding) hashes, slot growth and a small arena
# bound that forces rebuilds. Host-only, CPU-only.
$(BUILD)/answertab_check: native/server/answertab_check_main.cpp \
		native/server/answertab.hpp
	@mkdir -p $(BUILD)
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -Werror \
	    -fsanitize=address,undefined -fno-sanitize-recover=all \
	    $< -o $@

check-answertab: $(BUILD)/answertab_check
	$(BUILD)/answertab_check 1 100000

# Sanitizer run of the balancer's reply-run grouping (replyruns.hpp) in a
# stand-alone program with a recording sink: fixed and seeded random
# reply sequences, sinks that fail runs. Host-only, CPU-only.
$(BUILD)/replyruns_check: native/balancer/replyruns_check_main.cpp \
		native/balancer/replyruns.hpp
	@mkdir -p $(BUILD)
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -Werror \
	    -fsanitize=address,undefined -fno-sanitize-recover=all \
	    $< -o $@

check-replyruns: $(BUILD)/replyruns_check
	$(BUILD)/replyruns_check 1 300

# Sanitizer runs of the shared-memory byte rings (shmpipe.hpp) in a
# stand-alone program whose producer and consumer are two of its own
# threads: once under ASan+UBSan, once under ThreadSanitizer. Random
# chunks through a 4 KiB ring, full/partial/resume, the park/doorbell
# handshake over 100000 handoffs with bounded waits, corrupted control
# blocks. Host-only, CPU-only.
SHMPIPE_CHECK_DEPS := native/common/shmpipe_check_main.cpp \
	native/common/shmpipe.hpp

$(BUILD)/shmpipe_check_asan: $(SHMPIPE_CHECK_DEPS)
	@mkdir -p $(BUILD)
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -Werror \
	    -fsanitize=address,undefined -fno-sanitize-recover=all \
	    $< -o $@ -lpthread

$(BUILD)/shmpipe_check_tsan: $(SHMPIPE_CHECK_DEPS)
	@mkdir -p $(BUILD)
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -Werror \
	    -fsanitize=thread $< -o $@ -lpthread

check-shmpipe: $(BUILD)/shmpipe_check_asan $(BUILD)/shmpipe_check_tsan
	$(BUILD)/shmpipe_check_asan 1 100000
	$(BUILD)/shmpipe_check_tsan 1 100000

# Sanitizer run of the bsock1 transport endpoint (bsocklink.hpp) in a
# stand-alone program: two endpoints over a socketpair and 4 KiB rings,
# recording sinks; byte order across the stream-to-ring switch in both
# directions, stream and ring back-pressure, corrupted ring indices, the
# stream after the switch, an offer never answered. Host-only, CPU-only.
$(BUILD)/bsocklink_check: native/common/bsocklink_check_main.cpp \
		native/common/bsocklink.hpp native/common/shmpipe.hpp \
		native/server/framebuf.hpp native/balancer/protocol.hpp
	@mkdir -p $(BUILD)
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -Werror \
	    -fsanitize=address,undefined -fno-sanitize-recover=all \
	    $< -o $@

check-bsocklink: $(BUILD)/bsocklink_check
	$(BUILD)/bsocklink_check 1

# Sanitizer run of the ZooKeeper connect-string parser (zk/hostlist.hpp)
# in a stand-alone program: a fixed accept/reject table and seeded random
# strings, each parsed from a heap block of exactly its length; what is
# accepted is printed and parsed again and must give the same list.
# Host-only, CPU-only.
$(BUILD)/hostlist_check: native/zk/hostlist_check_main.cpp \
		native/zk/hostlist.hpp
	@mkdir -p $(BUILD)
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -Werror \
	    -fsanitize=address,undefined -fno-sanitize-recover=all \
	    $< -o $@

check-zkhosts: $(BUILD)/hostlist_check
	$(BUILD)/hostlist_check 1 20000

# ThreadSanitizer run of the serving-thread pool: binderd itself (a daemon
# with its own main) built with -fsanitize=thread into $(BUILD)/tsan, and
# the pool's tests plus the two suites that pin reply order and ingress
# run against it. The tests fail on any ThreadSanitizer report in a
# daemon's log. Host-only, CPU-only.
TSAN_FLAGS := -O1 -g -std=c++20 -fsanitize=thread -fno-omit-frame-pointer \
	-Wall -Wextra -Werror -Wno-unused-parameter
TSAN_SRCS := $(CORE_SRCS) $(SERVER_SRCS) native/server/binderd_main.cpp
TSAN_OBJS := $(TSAN_SRCS:%.cpp=$(BUILD)/tsan/obj/%.o)

$(BUILD)/tsan/obj/%.o: %.cpp
	@mkdir -p $(dir $@)
	$(CXX) $(TSAN_FLAGS) -MMD -MP -c $< -o $@

$(BUILD)/tsan/binderd: $(TSAN_OBJS)
	$(CXX) $(TSAN_FLAGS) $^ -o $@ -lssl -lcrypto -lpthread

check-serve-threads: all $(BUILD)/tsan/binderd
	BINDERD_BIN=$(CURDIR)/$(BUILD)/tsan/binderd $(PYTHON) -m pytest -q \
	    tests/test_serve_threads.py tests/test_answer_table.py \
	    tests/test_bsock_ingress.py

# Sanitizer run of the DNS codec (dns/codec.cpp) in a stand-alone
# program: a seeded corpus of encoded messages of every record type,
# their prefixes, mutations and random buffers, each decoded from a heap
# block of exactly its length; what decodes is re-encoded and must decode
# to the same message. Host-only, CPU-only.
$(BUILD)/codec_check: native/dns/codec_check_main.cpp native/dns/codec.cpp \
		native/dns/codec.hpp
	@mkdir -p $(BUILD)
	$(CXX) -O1 -g -std=c++20 -Wall -Wextra -Werror \
	    -fsanitize=address,undefined -fno-sanitize-recover=all \
	    native/dns/codec_check_main.cpp native/dns/codec.cpp -o $@

check-codec: $(BUILD)/codec_check
	$(BUILD)/codec_check 1 20

# AddressSanitizer+UBSan run of the served wire: binderd itself (a daemon
# with its own main) built with -fsanitize=address,undefined into
# $(BUILD)/asan, and the suites that put hand-built and hostile queries
# on its sockets run against it. The balancer and the Python side are
# the ordinary builds. tests/test_dns_wire_served.py fails on a sanitizer
# report in a daemon's log or a daemon that exited on its own. Host-only,
# CPU-only.
ASAN_FLAGS := -O1 -g -std=c++20 -fsanitize=address,undefined \
	-fno-sanitize-recover=all -fno-omit-frame-pointer \
	-Wall -Wextra -Werror -Wno-unused-parameter
ASAN_OBJS := $(TSAN_SRCS:%.cpp=$(BUILD)/asan/obj/%.o)

$(BUILD)/asan/obj/%.o: %.cpp
	@mkdir -p $(dir $@)
	$(CXX) $(ASAN_FLAGS) -MMD -MP -c $< -o $@

$(BUILD)/asan/binderd: $(ASAN_OBJS)
	$(CXX) $(ASAN_FLAGS) $^ -o $@ -lssl -lcrypto -lpthread

check-wire-asan: all $(BUILD)/asan/binderd
	BINDERD_BIN=$(CURDIR)/$(BUILD)/asan/binderd $(PYTHON) -m pytest -q \
	    tests/test_dns_wire_served.py tests/test_hostile_inputs.py \
	    tests/test_fastpath.py

# release tarball layout under /opt/binder-amd (the reference ships
# /opt/smartdc/binder with balancer+smf_adjust in lib/ and zklog in
# bin/; Makefile:178-229 there)
release: all
	rm -rf dist/binder-amd
	mkdir -p dist/binder-amd/bin dist/binder-amd/etc
	cp bin/binderd bin/binder-balancer bin/binder-adjust \
	    bin/zkd \
	    bin/binder-supervisor bin/zklogcat bin/dnsblast bin/zktool \
	    dist/binder-amd/bin/
	cp -r deploy dist/binder-amd/
	cp -r tools dist/binder-amd/
	cp etc/config.json.in etc/config.sample.json dist/binder-amd/etc/
	mkdir -p dist/binder-amd/lib/python/binder_amd
	cp binder_amd/*.py $(PYMOD) dist/binder-amd/lib/python/binder_amd/
	cp README.md LICENSE dist/binder-amd/
	cp -r docs dist/binder-amd/
	tar -C dist -czf dist/binder-amd.tar.gz binder-amd
	@echo "release: dist/binder-amd.tar.gz"

clean:
	rm -rf $(BUILD) $(PYMOD) $(BINARIES) dist

-include $(shell find $(BUILD) -name '*.d' 2>/dev/null)

.PHONY: all clean test check check-framebuf check-answertab \
	check-replyruns check-shmpipe check-bsocklink check-serve-threads \
	check-codec check-wire-asan check-zkhosts release
