# Sanitizer build of librq's HOST code (graph build, plan, workspace / ABI validation,
# the pinned staging ring): every -fsanitize applies to the host compilation only
# (-Xarch_host); the gfx950 device code is the normal build.  The source and header
# lists and the rules are the Makefile's.
#   make -f asan.mk     ->  ../_asan/librq.so
OUT = ../_asan/librq.so
BUILD = build_asan
include Makefile
HSAN = -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
       -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer
FLAGS = -O2 -g --offload-arch=$(ARCH) -ffp-contract=off -fno-fast-math -fPIC -std=c++17 $(HSAN)
LDFLAGS = -Xarch_host -shared-libsan $(HSAN)
